// query.hip -- ray queries on caller rays (include/rayrs_hip.h RAY QUERIES).  The kernels are not part of a render: a
// query is the render's Bvh::intersect on a ray the caller made, answered with the device functions the path kernels use
// (device_path.h) in a unit of its own, so that no path kernel is touched.
#include <hip/hip_runtime.h>

#include "device_path.h"
#include "launch_dispatch.h"
#include "query_kernels.h"

namespace rayrs {

// A ray is used as given: three f64 each, nothing normalised, any value.
RR_DEV void query_ray(const QueryDev& q, uint32_t i, V3& o, V3& d) {
    const double* po = q.origin + (size_t)i * 3u;
    const double* pd = q.direction + (size_t)i * 3u;
    o = mk(po[0], po[1], po[2]), d = mk(pd[0], pd[1], pd[2]);
}

// One ray per lane, as the self-test kernel of kernels.hip walks: the lanes past the end of the batch leave before the
// query, and the wave-level votes inside it are taken over the lanes that are there.  The closest hit's normal is
// FEATURES' normal_s, formed as features.hip forms it; the depth-first slot becomes the object on the device.
template <bool COMPACT>
__global__ void __launch_bounds__(256) query_intersect_kernel(SceneDev sc, QueryDev q) {
    extern __shared__ uint32_t lds_stack[];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const LaneStack stack = lane_stack(lds_stack, q.spill, sc);
    if (i >= q.n) return;
    V3 o, d;
    query_ray(q, i, o, d);
    double t = 0.0;
    uint32_t prim = 0xffffffffu;
    const bool hit = lane_query<COMPACT>(sc, o, d, stack, t, prim) && prim < q.n_prims;
    V3 n = mk(0.0, 0.0, 0.0);
    if (hit && q.normal != nullptr) {
        const PrimRec<COMPACT> rec = load_prim<COMPACT>(sc.prims, prim);
        n = hit_point<COMPACT>(rec, hit_position(o, d, t), d).normal;  // obj.geom.normal(r.point(t)): not flipped
    }
    q.t[i] = hit ? t : 0.0;
    q.object[i] = hit ? q.prim_object[prim] : 0xffffffffu;
    if (q.normal != nullptr) {
        double* dst = q.normal + (size_t)i * 3u;
        dst[0] = n.x, dst[1] = n.y, dst[2] = n.z;
    }
}

// The any-hit walk (device_path.h bvh_occluded), by the tree the scene names: sc.exact is the default walk's tree, with its
// hot group where the scene has one; else the tree of single primitives behind their own boxes, nothing culled either.
// STEPS: the lab's instance, which also stores how many turns of the walk's loop each ray took.
template <bool COMPACT, bool STEPS>
__global__ void __launch_bounds__(256) query_occluded_kernel(SceneDev sc, QueryDev q) {
    extern __shared__ uint32_t lds_stack[];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const LaneStack stack = lane_stack(lds_stack, q.spill, sc);
    if (i >= q.n) return;
    V3 o, d;
    query_ray(q, i, o, d);
    const double t_max = q.t_max != nullptr ? q.t_max[i] : (double)__builtin_inf();
    uint32_t steps = 0u;
    const bool found = sc.exact ? bvh_occluded<COMPACT, true, STEPS>(sc, o, d, t_max, stack, &steps)
                                : bvh_occluded<COMPACT, false, STEPS>(sc, o, d, t_max, stack, &steps);
    q.occluded[i] = found ? (uint8_t)1 : (uint8_t)0;
    if (STEPS) q.steps[i] = steps;
}

template <class K, class... Bools>
static hipError_t launch_query(K kernel_of, const SceneDev& sc, const QueryDev& q, hipStream_t stream, Bools... bools) {
    if (q.n == 0u) return hipSuccess;
    const uint32_t lds = lane_stacks_lds_bytes(sc.stack_lds);
    const uint32_t blocks = (uint32_t)(query_threads(q.n) / 256u);
    return with_bools([&](auto... cs) {
        auto kernel = kernel_of(cs...);
        const hipError_t e = raise_dynamic_lds(kernel, lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), lds, stream, sc, q);
        return hipGetLastError();
    }, bools...);
}

hipError_t launch_query_intersect(bool compact, const SceneDev& sc, const QueryDev& q, hipStream_t stream) {
    return launch_query([](auto C) { return &query_intersect_kernel<decltype(C)::value>; }, sc, q, stream, compact);
}

hipError_t launch_query_occluded(bool compact, const SceneDev& sc, const QueryDev& q, hipStream_t stream) {
    return launch_query([](auto C, auto S) { return &query_occluded_kernel<decltype(C)::value, decltype(S)::value>; }, sc, q, stream,
                        compact, q.steps != nullptr);
}

}  // namespace rayrs
