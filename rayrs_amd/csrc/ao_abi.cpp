// ao_abi.cpp -- ambient occlusion of include/rayrs_hip.h (AMBIENT OCCLUSION): the refusals, a batch of points through
// launches of ao.hip's kernel on the caller's stream, the host form around them (upload, launch, wait, download), the image
// form (a first pass that leaves every pixel's point on the device, then the same launches), and the lab's hooks
// (rayrs_lab.h rayrs_lab_ao_refill, rayrs_lab_ao_turns).
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/rayrs_hip.h"
#include "ao_kernels.h"
#include "features_host.hpp"
#include "scene_internal.hpp"

using namespace rayrs;

namespace {

// The refusals that need no device, in the header's order.
int ao_check(const rayrs_scene* scene, const void* position, const void* normal, const void* count, const void* visibility,
             uint32_t samples, uint32_t fast_traversal) {
    if (!scene || !position || !normal || (!count && !visibility)) return RAYRS_INVALID_ARG;
    if (samples == 0u || fast_traversal > 1u) return RAYRS_INVALID_ARG;
    if (scene->device < 0) return RAYRS_NO_DEVICE;
    return RAYRS_OK;
}

// The queries' stack strip (scene_internal.hpp rayrs_scene::Queries), taken and handed back as query_abi.cpp's
// query_enqueue does: reserved at a launch's largest size, and a user on another stream waits on the device for the last one.
int strip_take(rayrs_scene* scene, const SceneDev& sc, hipStream_t stream, uint32_t** spill) {
    rayrs_scene::Queries& own = scene->queries;
    if (sc.stack_depth > sc.stack_lds) {
        HIP_TRY(own.d_stack_spill.reserve(stack_spill_words(sc, QUERY_LAUNCH_RAYS) * sizeof(uint32_t)));
        if (!own.has_event) {
            HIP_TRY(own.ev_done.create());
            own.has_event = true;
        }
        if (own.strip_in_use) HIP_TRY(hipStreamWaitEvent(stream, own.ev_done, 0));
    }
    *spill = own.d_stack_spill.as<uint32_t>();
    return RAYRS_OK;
}
int strip_give_back(rayrs_scene* scene, const SceneDev& sc, hipStream_t stream) {
    rayrs_scene::Queries& own = scene->queries;
    if (sc.stack_depth > sc.stack_lds) {
        HIP_TRY(hipEventRecord(own.ev_done, stream));
        own.strip_in_use = true;
    }
    return RAYRS_OK;
}

// The batch, at most ao_launch_points(samples) points per launch, all on `stream`: `ao` holds the whole batch's pointers,
// which move on from launch to launch, and index_base with them.  fast_traversal is taken as asked.
int ao_enqueue(rayrs_scene* scene, uint32_t fast_traversal, uint64_t n, AoDev ao, hipStream_t stream) {
    const SceneDev sc = make_scene_dev(scene, fast_traversal == 0u);
    ao.block_points = ao_block_points(ao.samples);
    ao.refill_below = scene->ao.refill_below ? scene->ao.refill_below : AO_REFILL_BELOW;
    RAYRS_TRY(strip_take(scene, sc, stream, &ao.spill));
    const uint64_t per_launch = ao_launch_points(ao.samples);
    for (uint64_t base = 0; base < n; base += per_launch) {
        AoDev part = ao;
        part.n = (uint32_t)(n - base < per_launch ? n - base : per_launch);
        part.index_base = ao.index_base + base;
        part.position = ao.position + base * 3u, part.normal = ao.normal + base * 3u;
        part.active = ao.active ? ao.active + base : nullptr;
        part.count = ao.count ? ao.count + base : nullptr;
        part.visibility = ao.visibility ? ao.visibility + base : nullptr;
        HIP_TRY(launch_ao(scene->flat.compact, sc, part, stream));
    }
    return strip_give_back(scene, sc, stream);
}

AoDev ao_args(const double* position, const double* normal, uint32_t samples, double t_max, double bias, uint64_t seed,
              uint64_t index_base, uint32_t* count, double* visibility) {
    AoDev ao;
    std::memset(&ao, 0, sizeof(ao));
    ao.samples = samples, ao.seed = seed, ao.index_base = index_base;
    ao.t_max = t_max, ao.bias = bias;
    ao.position = position, ao.normal = normal;
    ao.count = count, ao.visibility = visibility;
    return ao;
}

// The host form -- upload, launch on the null stream, wait, download -- and the lab's with `turns`.
int ao_host(rayrs_scene* scene, const double* position, const double* normal, uint64_t n, uint32_t samples, double t_max, double bias,
            uint64_t seed, uint64_t index_base, uint32_t fast_traversal, uint32_t* count, double* visibility,
            unsigned long long* turns) {
    HIP_TRY(hipSetDevice(scene->device));
    rayrs_scene::Ao& own = scene->ao;
    HIP_TRY(own.d_position.upload(position, n * 3u * sizeof(double)));
    HIP_TRY(own.d_normal.upload(normal, n * 3u * sizeof(double)));
    if (count) HIP_TRY(own.d_count.reserve(n * sizeof(uint32_t)));
    if (visibility) HIP_TRY(own.d_visibility.reserve(n * sizeof(double)));
    AoDev ao = ao_args(own.d_position.as<double>(), own.d_normal.as<double>(), samples, t_max, bias, seed, index_base,
                       count ? own.d_count.as<uint32_t>() : nullptr, visibility ? own.d_visibility.as<double>() : nullptr);
    if (turns) {
        HIP_TRY(own.d_turns.reserve(2u * sizeof(unsigned long long)));
        HIP_TRY(hipMemsetAsync(own.d_turns.as<>(), 0, 2u * sizeof(unsigned long long), nullptr));
        ao.turns = own.d_turns.as<unsigned long long>();
    }
    RAYRS_TRY(ao_enqueue(scene, fast_traversal, n, ao, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    if (count) HIP_TRY(own.d_count.download(count, n * sizeof(uint32_t)));
    if (visibility) HIP_TRY(own.d_visibility.download(visibility, n * sizeof(double)));
    if (turns) HIP_TRY(own.d_turns.download(turns, 2u * sizeof(unsigned long long)));
    return RAYRS_OK;
}

}  // namespace

extern "C" {

int rayrs_scene_ambient_occlusion_launch(rayrs_scene* scene, const double* position, const double* normal, uint64_t n, uint32_t samples,
                                         double t_max, double bias, uint64_t seed, uint64_t index_base, uint32_t fast_traversal,
                                         uint32_t* count, double* visibility, void* hip_stream) {
    RAYRS_GUARDED({
    RAYRS_TRY(ao_check(scene, position, normal, count, visibility, samples, fast_traversal));
    if (n == 0u) return RAYRS_OK;
    HIP_TRY(hipSetDevice(scene->device));
    return ao_enqueue(scene, fast_traversal, n, ao_args(position, normal, samples, t_max, bias, seed, index_base, count, visibility),
                      reinterpret_cast<hipStream_t>(hip_stream));
    })
}

int rayrs_scene_ambient_occlusion(rayrs_scene* scene, const double* position, const double* normal, uint64_t n, uint32_t samples,
                                  double t_max, double bias, uint64_t seed, uint64_t index_base, uint32_t fast_traversal,
                                  uint32_t* count, double* visibility) {
    RAYRS_GUARDED({
    RAYRS_TRY(ao_check(scene, position, normal, count, visibility, samples, fast_traversal));
    if (n == 0u) return RAYRS_OK;
    return ao_host(scene, position, normal, n, samples, t_max, bias, seed, index_base, fast_traversal, count, visibility, nullptr);
    })
}

int rayrs_render_ao(rayrs_scene* scene, const rayrs_camera* camera, uint64_t seed, uint64_t ao_seed, uint32_t samples, double t_max,
                    double bias, uint32_t fast_traversal, uint32_t* count, double* visibility) {
    RAYRS_GUARDED({
    if (!scene || !camera || (!count && !visibility)) return RAYRS_INVALID_ARG;
    if (samples == 0u) return RAYRS_INVALID_ARG;
    RAYRS_TRY(features_check(camera, 1u, 0u, 1u, fast_traversal));  // (the camera's refusals are FEATURES')
    if (scene->device < 0) return RAYRS_NO_DEVICE;
    RAYRS_TRY(scene_settle(scene));
    rayrs_scene::Ao& own = scene->ao;
    const size_t npix = (size_t)camera->x_pixels * camera->y_pixels;
    HIP_TRY(own.d_position.reserve(npix * 3u * sizeof(double)));
    HIP_TRY(own.d_normal.reserve(npix * 3u * sizeof(double)));
    HIP_TRY(own.d_active.reserve(npix));
    if (count) HIP_TRY(own.d_count.reserve(npix * sizeof(uint32_t)));
    if (visibility) HIP_TRY(own.d_visibility.reserve(npix * sizeof(double)));
    {
        // the primary rays' query is the render's, by the walk a render with these settings takes (as features_abi.cpp)
        const FrameWalk walk = frame_walk(scene, camera, fast_traversal);
        const SceneDev sc = make_scene_dev(scene, walk.exact || walk.use_local);
        const CameraDev cam = make_camera_dev(camera);
        AoPrimaryDev pd;
        std::memset(&pd, 0, sizeof(pd));
        pd.share = tile_share(camera->x_pixels, camera->y_pixels, 0u, 1u);
        pd.seed = seed;
        pd.position = own.d_position.as<double>(), pd.normal = own.d_normal.as<double>(), pd.active = own.d_active.as<uint8_t>();
        RAYRS_TRY(strip_take(scene, sc, nullptr, &pd.spill));
        const uint32_t per_launch = (uint32_t)(QUERY_LAUNCH_RAYS / 64u);  // tiles: one wave each
        for (uint32_t tile0 = 0; tile0 < pd.share.n_local_tiles; tile0 += per_launch) {
            pd.tile0 = tile0;
            pd.n_tiles = pd.share.n_local_tiles - tile0 < per_launch ? pd.share.n_local_tiles - tile0 : per_launch;
            HIP_TRY(launch_ao_primary(scene->flat.compact, sc, cam, pd, nullptr));
        }
        RAYRS_TRY(strip_give_back(scene, sc, nullptr));
    }
    AoDev ao = ao_args(own.d_position.as<double>(), own.d_normal.as<double>(), samples, t_max, bias, ao_seed, 0u,
                       count ? own.d_count.as<uint32_t>() : nullptr, visibility ? own.d_visibility.as<double>() : nullptr);
    ao.active = own.d_active.as<uint8_t>();
    RAYRS_TRY(ao_enqueue(scene, fast_traversal, npix, ao, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    if (count) HIP_TRY(own.d_count.download(count, npix * sizeof(uint32_t)));
    if (visibility) HIP_TRY(own.d_visibility.download(visibility, npix * sizeof(double)));
    return RAYRS_OK;
    })
}

int rayrs_lab_ao_refill(rayrs_scene* scene, uint32_t refill_below) {
    if (!scene || refill_below > 64u) return RAYRS_INVALID_ARG;
    scene->ao.refill_below = refill_below;
    return RAYRS_OK;
}

int rayrs_lab_ao_turns(rayrs_scene* scene, const double* position, const double* normal, uint64_t n, uint32_t samples, double t_max,
                       double bias, uint64_t seed, uint64_t index_base, uint32_t fast_traversal, uint32_t* count, uint64_t turns[2]) {
    RAYRS_GUARDED({
    RAYRS_TRY(ao_check(scene, position, normal, count, turns, samples, fast_traversal));
    if (!count || !turns) return RAYRS_INVALID_ARG;
    turns[0] = turns[1] = 0u;
    if (n == 0u) return RAYRS_OK;
    unsigned long long got[2] = {0ull, 0ull};
    RAYRS_TRY(ao_host(scene, position, normal, n, samples, t_max, bias, seed, index_base, fast_traversal, count, nullptr, got));
    turns[0] = got[0], turns[1] = got[1];
    return RAYRS_OK;
    })
}

}  // extern "C"
