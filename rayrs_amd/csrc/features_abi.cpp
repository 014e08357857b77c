// features_abi.cpp -- first-hit feature buffers of include/rayrs_hip.h (rayrs_render_features) and what film_abi.cpp's
// rayrs_film_features and filters share with it: the refusals, a features pass into device planes (features.hip), the
// copy to the host.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "../../include/rayrs_hip.h"
#include "features_host.hpp"

using namespace rayrs;

namespace rayrs {

int features_check(const rayrs_camera* camera, uint32_t samples, uint32_t tile_rank, uint32_t tile_ranks, uint32_t fast_traversal) {
    if (!camera || samples == 0u || samples > SLOT_SAMPLE_MASK) return RAYRS_INVALID_ARG;  // (a sample index has 30 bits, as a render's)
    if (tile_ranks == 0u || tile_rank >= tile_ranks || fast_traversal > 1u) return RAYRS_INVALID_ARG;
    if (camera->x_pixels == 0u || camera->y_pixels == 0u) return RAYRS_INVALID_ARG;
    if (camera->x_pixels > 65535u || camera->y_pixels > 65535u) return RAYRS_UNSUPPORTED;
    return RAYRS_OK;
}

int features_run(rayrs_scene* scene, const rayrs_camera* camera, uint32_t samples, uint64_t seed, uint32_t tile_rank,
                 uint32_t tile_ranks, uint32_t fast_traversal, FeatureBufs& b) {
    const size_t npix = (size_t)camera->x_pixels * camera->y_pixels;
    HIP_TRY(b.normal.reserve(npix * 3 * sizeof(double)));
    HIP_TRY(b.albedo.reserve(npix * 3 * sizeof(double)));
    HIP_TRY(b.depth.reserve(npix * sizeof(double)));
    HIP_TRY(b.coverage.reserve(npix * sizeof(double)));
    HIP_TRY(b.prim.reserve(npix * sizeof(uint32_t)));
    // pixels outside the share read +0 and 0xffffffff
    HIP_TRY(hipMemsetAsync(b.normal.as<>(), 0, npix * 3 * sizeof(double), nullptr));
    HIP_TRY(hipMemsetAsync(b.albedo.as<>(), 0, npix * 3 * sizeof(double), nullptr));
    HIP_TRY(hipMemsetAsync(b.depth.as<>(), 0, npix * sizeof(double), nullptr));
    HIP_TRY(hipMemsetAsync(b.coverage.as<>(), 0, npix * sizeof(double), nullptr));
    HIP_TRY(hipMemsetAsync(b.prim.as<>(), 0xff, npix * sizeof(uint32_t), nullptr));
    // the walk a render with these settings takes: a local-pool scene never makes the fast walk's bets
    const FrameWalk walk = frame_walk(scene, camera, fast_traversal);
    const SceneDev sc = make_scene_dev(scene, walk.exact || walk.use_local);
    const CameraDev cam = make_camera_dev(camera);
    FeatureDev fd;
    std::memset(&fd, 0, sizeof(fd));
    fd.samples = samples;
    fd.share = tile_share(camera->x_pixels, camera->y_pixels, tile_rank, tile_ranks);
    fd.seed = seed;
    fd.inv_samples = 1.0 / (double)samples;
    fd.normal = b.normal.as<double>(), fd.albedo = b.albedo.as<double>();
    fd.depth = b.depth.as<double>(), fd.coverage = b.coverage.as<double>();
    fd.prim = b.prim.as<uint32_t>();
    if (sc.stack_depth > sc.stack_lds)
        HIP_TRY(b.spill.reserve(stack_spill_words(sc, features_threads(fd.share.n_local_tiles)) * sizeof(uint32_t)));
    fd.spill = b.spill.as<uint32_t>();
    HIP_TRY(launch_features(scene->flat.compact, sc, cam, fd, nullptr));
    return RAYRS_OK;
}

int features_download(const rayrs_scene* scene, const rayrs_camera* camera, const FeatureBufs& b, double* normal, double* albedo,
                      double* depth, double* coverage, uint32_t* object) {
    const size_t npix = (size_t)camera->x_pixels * camera->y_pixels;
    if (normal) HIP_TRY(b.normal.download(normal, npix * 3 * sizeof(double)));
    if (albedo) HIP_TRY(b.albedo.download(albedo, npix * 3 * sizeof(double)));
    if (depth) HIP_TRY(b.depth.download(depth, npix * sizeof(double)));
    if (coverage) HIP_TRY(b.coverage.download(coverage, npix * sizeof(double)));
    if (object) {
        HIP_TRY(b.prim.download(object, npix * sizeof(uint32_t)));
        const std::vector<uint32_t>& prim_object = scene->flat.prim_object;  // depth-first slot -> object in insertion order
        for (size_t k = 0; k < npix; k++)
            if (object[k] != 0xffffffffu) object[k] = object[k] < prim_object.size() ? prim_object[object[k]] : 0xffffffffu;
    }
    if (!normal && !albedo && !depth && !coverage && !object) HIP_TRY(hipStreamSynchronize(nullptr));
    return RAYRS_OK;
}

}  // namespace rayrs

extern "C" {

int rayrs_render_features(rayrs_scene* scene, const rayrs_camera* camera, uint32_t samples, uint64_t seed, uint32_t tile_rank,
                          uint32_t tile_ranks, uint32_t fast_traversal, double* normal, double* albedo, double* depth,
                          double* coverage, uint32_t* object) {
    RAYRS_GUARDED({
    if (!scene || !camera) return RAYRS_INVALID_ARG;
    RAYRS_TRY(features_check(camera, samples, tile_rank, tile_ranks, fast_traversal));
    if (scene->device < 0) return RAYRS_NO_DEVICE;
    RAYRS_TRY(scene_settle(scene));
    FeatureBufs b;
    RAYRS_TRY(features_run(scene, camera, samples, seed, tile_rank, tile_ranks, fast_traversal, b));
    RAYRS_TRY(features_download(scene, camera, b, normal, albedo, depth, coverage, object));
    return RAYRS_OK;
    })
}

}  // extern "C"
