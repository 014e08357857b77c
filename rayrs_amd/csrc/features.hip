// features.hip -- first-hit feature buffers (include/rayrs_hip.h FEATURES).  The kernel is not part of a render: the
// features of a sample depend on (scene, camera, seed, pixel, sample index) only, so they are recomputed here from the
// device functions the path kernels use (device_path.h) instead of being carried through the path rounds, whose kernels
// sit at their register bound.
#include <hip/hip_runtime.h>

#include "device_path.h"
#include "feature_kernels.h"

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
    const uint32_t wave = threadIdx.x >> 6;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    // sc.stack_lds entries of the stack in LDS, the rest in the strip `spill` (as in the traversal kernel)
    const LaneStack stack{lds_stack + (size_t)wave * (sc.stack_lds + 1u) * 64u + lane, fd.spill + i, sc.stack_lds,
                          gridDim.x * blockDim.x};
    const TilePixel px = tile_pixel(fd.share, (uint32_t)(i >> 6), lane);
    if (!px.in_share) return;  // (wave-uniform)
    const bool inside = px.row < cam.H && px.col < cam.W;
    const uint32_t r = px.row < cam.H ? px.row : cam.H - 1u, c = px.col < cam.W ? px.col : cam.W - 1u;
    const uint64_t pixel = (uint64_t)r * cam.W + c;
    V3 n_sum = mk(0.0, 0.0, 0.0), a_sum = mk(0.0, 0.0, 0.0);
    double z_sum = 0.0, cov_sum = 0.0;
    uint32_t first_prim = 0xffffffffu;
    for (uint32_t s = 0; s < fd.samples; s++) {
        Rng rng{rr_path_key(fd.seed, pixel, (uint64_t)s), 0};
        V3 o, d;
        primary_ray(cam, cam.H - r, cam.W - c, rng, o, d);  // image origin is upper left, camera origin lower right (main.rs:74-75)
        double t = 0.0;
        uint32_t prim = 0xffffffffu;
        WorkCount wc{0, 0, 0, 0, 0};
        const bool hit = sc.exact ? bvh_intersect<COMPACT, false, true>(sc, o, d, stack, t, prim, wc)
                                  : bvh_intersect<COMPACT, false, false>(sc, o, d, stack, t, prim, wc);
        V3 n = mk(0.0, 0.0, 0.0), a = mk(0.0, 0.0, 0.0);
        double z = 0.0, cov = 0.0;
        if (hit) {
            const PrimRec<COMPACT> rec = load_prim<COMPACT>(sc.prims, prim);
            const V3 position = v_add(o, v_scale(d, t));
            n = prim_normal<COMPACT>(rec, position);  // what radiance hands to Material::evaluate (lib.rs:528-529): not flipped
            const SurfaceDev* surf = sc.surfaces + (rec.tag() >> 8);
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
    const uint32_t lds = 4u * 64u * (sc.stack_lds + 1u) * 4u;  // four waves' stacks, + the spare entry
    const uint32_t blocks = (uint32_t)(features_threads(fd.share.n_local_tiles) / 256u);
    if (compact) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&features_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds);
        hipLaunchKernelGGL(features_kernel<true>, dim3(blocks), dim3(256), lds, stream, sc, cam, fd);
    } else {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&features_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds);
        hipLaunchKernelGGL(features_kernel<false>, dim3(blocks), dim3(256), lds, stream, sc, cam, fd);
    }
    return hipGetLastError();
}

}  // namespace rayrs
