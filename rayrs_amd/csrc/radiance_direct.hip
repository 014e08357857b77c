// radiance_direct.hip -- the radiance queries with direct lighting (include/rayrs_hip.h DIRECT LIGHTING).  A unit of its own
// beside radiance_lit.hip: the kernels of the queries' three starts, the resolve and the launch.  The wave itself -- a lane walks
// TWO rays per diffuse bounce, the shadow ray and then the continuation -- is radiance_direct_wave.h's, which the direct-lit
// film's kernels (film_direct.hip) run with a start of their own.
#include <hip/hip_runtime.h>

#include "device_path.h"
#include "launch_dispatch.h"
#include "radiance_direct_kernels.h"
#include "radiance_direct_wave.h"

namespace rayrs {

// radiance_direct_wave.h's wave, its paths started by the queries: a batch's rays, points or pixels.
template <bool COMPACT, bool EXACT, int START>
__global__ void __launch_bounds__(256) radiance_direct_kernel(SceneDev sc, RadianceDev rd, LightsDev lights, LightSlotsDev slots, CameraDev cam) {
    extern __shared__ uint32_t lds_stack[];
    direct_wave<COMPACT, EXACT>(QueryStart<START>{}, lane_stack(lds_stack, rd.spill, sc), sc, rd, lights, slots, cam);
}

// A ray's chunk sums added in chunk order (the first assigned), scaled by the reciprocal of S, and its query counts added:
// one thread per ray.
__global__ void __launch_bounds__(256) radiance_direct_resolve_kernel(RadianceDev rd) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= rd.n) return;
    const double* p = rd.partial + (size_t)i * rd.chunks * 3u;
    const uint32_t* pq = rd.partial_queries + (size_t)i * rd.chunks;
    V3 sum = mk(p[0], p[1], p[2]);
    uint32_t q = pq[0];
    for (uint32_t k = 1; k < rd.chunks; k++) {
        sum = v_add(sum, mk(p[3u * k], p[3u * k + 1u], p[3u * k + 2u]));
        q += pq[k];
    }
    const double inv = 1.0 / (double)rd.samples;
    if (rd.radiance != nullptr) {
        double* dst = rd.radiance + (size_t)i * 3u;
        dst[0] = sum.x * inv, dst[1] = sum.y * inv, dst[2] = sum.z * inv;
    }
    if (rd.queries != nullptr) rd.queries[i] = q;
}

namespace {

template <int START>
hipError_t launch_direct_start(bool compact, const SceneDev& sc, const RadianceDev& rd, const LightsDev& lights, const LightSlotsDev& slots,
                               const CameraDev& cam, uint32_t blocks, uint32_t lds, hipStream_t stream) {
    return with_bools([&](auto C, auto E) {
        auto kernel = &radiance_direct_kernel<decltype(C)::value, decltype(E)::value, START>;
        const hipError_t e = raise_dynamic_lds(kernel, lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), lds, stream, sc, rd, lights, slots, cam);
        return hipGetLastError();
    }, compact, sc.exact != 0u);
}

}  // namespace

hipError_t launch_radiance_direct(bool compact, const SceneDev& sc, const RadianceDev& rd, const LightsDev& lights,
                                  const LightSlotsDev& slots, const CameraDev& cam, int start, int cu_count, hipStream_t stream) {
    if (rd.n == 0u) return hipSuccess;
    const uint32_t lds = lane_stacks_lds_bytes(sc.stack_lds);
    const uint64_t n_items = (uint64_t)rd.n * rd.chunks;
    const uint64_t waves = (n_items + 63u) / 64u;  // (a wave takes up to 64 items at its first refill)
    uint64_t blocks = (uint64_t)(cu_count > 0 ? cu_count : 1) * RADIANCE_BLOCKS_PER_CU;
    if (blocks > QUERY_LAUNCH_RAYS / 256u) blocks = QUERY_LAUNCH_RAYS / 256u;  // (the stack strip is the queries')
    if (blocks > waves) blocks = waves;
    hipError_t e;
    if (start == LIT_START_PIXEL) e = launch_direct_start<LIT_START_PIXEL>(compact, sc, rd, lights, slots, cam, (uint32_t)blocks, lds, stream);
    else if (start == LIT_START_POINT) e = launch_direct_start<LIT_START_POINT>(compact, sc, rd, lights, slots, cam, (uint32_t)blocks, lds, stream);
    else e = launch_direct_start<LIT_START_RAY>(compact, sc, rd, lights, slots, cam, (uint32_t)blocks, lds, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(radiance_direct_resolve_kernel, dim3((rd.n + 255u) / 256u), dim3(256), 0, stream, rd);
    return hipGetLastError();
}

}  // namespace rayrs
