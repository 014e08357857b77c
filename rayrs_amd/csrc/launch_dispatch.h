// launch_dispatch.h -- what the launch glue of the .hip files shares: run-time bools into template arguments, a kernel's
// dynamic-LDS limit, and the LDS and the launch of a kernel whose lanes each walk the tree with a stack of their own.
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <mutex>
#include <type_traits>

namespace rayrs {

// with_bools(f, a, b, ...) calls f(A, B, ...) where A is std::true_type{} or std::false_type{} as a is true or false, and so
// on: inside f, A() is a constant expression and may pick a kernel template's instance.  Every combination of the
// bools is instantiated, so the kernels a launch wrapper can start are the ones its lambda names, for all values.
template <class F> auto with_bools(F f) { return f(); }
template <class F, class... Rest>
auto with_bools(F f, bool b, Rest... rest) {
    return b ? with_bools([&](auto... cs) { return f(std::true_type{}, cs...); }, rest...)
             : with_bools([&](auto... cs) { return f(std::false_type{}, cs...); }, rest...);
}

// A kernel's dynamic-LDS limit belongs to the kernel on a device, not to a scene or a launch, and every thread of the
// process that launches the kernel shares it: it is only ever raised, so that at every launch it is at least what the
// launch asks for -- set to each launch's own size, one thread could lower it between another's set and its launch.
template <class... Args>
hipError_t raise_dynamic_lds(void (*kernel_fn)(Args...), uint32_t lds) {
    static std::mutex mutex;  // (mutex and map are per kernel signature, which is enough: a kernel has one)
    static std::map<std::pair<int, const void*>, uint32_t> raised;  // (device, kernel): what its limit there was last set to
    const void* kernel = reinterpret_cast<const void*>(kernel_fn);
    int device = 0;
    hipError_t e = hipGetDevice(&device);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(mutex);
    uint32_t& set = raised[{device, kernel}];
    if (lds <= set) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) set = lds;
    return e;
}

// Dynamic LDS of a 256-thread workgroup of one-lane queries (device_path.h lane_stack): four waves' stacks of
// stack_lds entries and the spare one.
inline uint32_t lane_stacks_lds_bytes(uint32_t stack_lds) { return 4u * 64u * (stack_lds + 1u) * 4u; }

// The launch of such a kernel on `blocks` workgroups of 256: its dynamic-LDS limit raised to the stacks' size, then the launch.
template <class... Params, class... Args>
hipError_t launch_lane_stacks(void (*kernel)(Params...), uint32_t blocks, uint32_t stack_lds, hipStream_t stream, const Args&... args) {
    const uint32_t lds = lane_stacks_lds_bytes(stack_lds);
    const hipError_t e = raise_dynamic_lds(kernel, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), lds, stream, args...);
    return hipGetLastError();
}

}  // namespace rayrs
