// features.hip -- first-hit feature buffers (include/rayrs_hip.h FEATURES).  The kernel is not part of a render: the
// features of a sample depend on (scene, camera, seed, pixel, sample index) only, so they are recomputed here from the
// device functions the path kernels use (device_path.h) instead of being carried through the path rounds, whose kernels
// sit at their register bound.
#include <hip/hip_runtime.h>

#include "device_path.h"
#include "feature_kernels.h"
#include "launch_dispatch.h"

namespace rayrs {

// One wave per 8x8 tile of the share, one lane per pixel, as the film kernels map them: a wave's primary rays leave
// through neighbouring pixels and walk the same records.  A lane runs its pixel's samples in sample order with the eight
// running sums in registers -- the first sample's values assigned, the others added, f64, nothing fused -- and stores
// sum * (1 / samples).  The lanes of an edge tile's padding trace the nearest pixel of the image beside them and store
// nothing, so that every lane of a wave is in every query (the triangle and hot-group tests vote across the wave).
template <bool COMPACT>
__global__ void __launch_bounds__(256) features_kernel(SceneDev sc, CameraDev cam, FeatureDev fd) {
    extern __shared__ uint32_t lds_stack[];
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const LaneStack stack = lane_stack(lds_stack, fd.spill, sc);
    const TilePixel px = tile_pixel(fd.share, (uint32_t)(i >> 6), lane);
    if (!px.in_share) return;  // (wave-uniform)
    const bool inside = px.row < cam.H && px.col < cam.W;
    const uint32_t r = px.row < cam.H ? px.row : cam.H - 1u, c = px.col < cam.W ? px.col : cam.W - 1u;
    V3 n_sum = mk(0.0, 0.0, 0.0), a_sum = mk(0.0, 0.0, 0.0);
    double z_sum = 0.0, cov_sum = 0.0;
    uint32_t first_prim = 0xffffffffu;
    for (uint32_t s = 0; s < fd.samples; s++) {
        Rng rng{sample_key(fd.seed, cam, r, c, s), 0};
        V3 o, d;
        sample_ray(cam, r, c, rng, o, d);
        double t = 0.0;
        uint32_t prim = 0xffffffffu;
        const bool hit = lane_query<COMPACT>(sc, o, d, stack, t, prim);
        V3 n = mk(0.0, 0.0, 0.0), a = mk(0.0, 0.0, 0.0);
        double z = 0.0, cov = 0.0;
        if (hit) {
            const PrimRec<COMPACT> rec = load_prim<COMPACT>(sc.prims, prim);
            const HitPoint hp = hit_point<COMPACT>(rec, hit_position(o, d, t), d);
            n = hp.normal;  // what radiance hands to Material::evaluate (lib.rs:528-529): not flipped
            const SurfaceDev* surf = sc.surfaces + hp.sid;
            const int32_t kind = surf->kind;
            const double* col3 = kind >= RAYRS_MAT_COOK_TORRANCE && kind <= RAYRS_MAT_COOK_TORRANCE_GLASS ? surf->ct_color : surf->color;
            a = kind == RAYRS_MAT_NO_REFLECT ? mk(0.0, 0.0, 0.0) : mk(col3[0], col3[1], col3[2]);
            z = t, cov = 1.0;
        }
        if (s == 0u) {
            n_sum = n, a_sum = a, z_sum = z, cov_sum = cov;
            first_prim = hit ? prim : 0xffffffffu;
        } else {
            n_sum = v_add(n_sum, n), a_sum = v_add(a_sum, a);
            z_sum += z, cov_sum += cov;
        }
    }
    if (!inside) return;
    const size_t pix = (size_t)px.row * cam.W + px.col;
    const double inv = fd.inv_samples;
    fd.normal[3 * pix] = n_sum.x * inv, fd.normal[3 * pix + 1] = n_sum.y * inv, fd.normal[3 * pix + 2] = n_sum.z * inv;
    fd.albedo[3 * pix] = a_sum.x * inv, fd.albedo[3 * pix + 1] = a_sum.y * inv, fd.albedo[3 * pix + 2] = a_sum.z * inv;
    fd.depth[pix] = z_sum * inv;
    fd.coverage[pix] = cov_sum * inv;
    fd.prim[pix] = first_prim;
}

hipError_t launch_features(bool compact, const SceneDev& sc, const CameraDev& cam, const FeatureDev& fd, hipStream_t stream) {
    if (fd.share.n_local_tiles == 0u || fd.samples == 0u) return hipSuccess;
    const uint32_t lds = lane_stacks_lds_bytes(sc.stack_lds);
    const uint32_t blocks = (uint32_t)(features_threads(fd.share.n_local_tiles) / 256u);
    return with_bools([&](auto C) {
        const hipError_t e = raise_dynamic_lds(features_kernel<C()>, lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(features_kernel<C()>, dim3(blocks), dim3(256), lds, stream, sc, cam, fd);
        return hipGetLastError();
    }, compact);
}

}  // namespace rayrs
