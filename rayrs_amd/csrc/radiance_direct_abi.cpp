// radiance_direct_abi.cpp -- the radiance queries with direct lighting of include/rayrs_hip.h (DIRECT LIGHTING): the entry points.
// The refusals (the material rule among them), the light table, the launches and the host forms are the lit queries'
// (radiance_lit_abi.cpp), taken with LitCall::direct set.
#include <hip/hip_runtime.h>

#include "../../include/rayrs_hip.h"
#include "radiance_lit_host.hpp"

using namespace rayrs;

extern "C" {

int rayrs_scene_radiance_direct(rayrs_scene* scene, const double* origin, const double* direction, uint64_t n, uint32_t samples,
                                uint32_t max_bounces, uint32_t sample_chunk, uint64_t seed, uint64_t index_base, uint32_t fast_traversal,
                                const uint32_t* lights, uint32_t n_lights, double* radiance, uint32_t* queries) {
    RAYRS_GUARDED({
    return lit_entry(scene, LitCall{LIT_START_RAY, samples, max_bounces, sample_chunk, 0.0, seed, index_base, fast_traversal, lights, n_lights, true},
                     origin, direction, n, radiance, queries, false, nullptr);
    })
}

int rayrs_scene_radiance_direct_launch(rayrs_scene* scene, const double* origin, const double* direction, uint64_t n, uint32_t samples,
                                       uint32_t max_bounces, uint32_t sample_chunk, uint64_t seed, uint64_t index_base,
                                       uint32_t fast_traversal, const uint32_t* lights, uint32_t n_lights, double* radiance,
                                       uint32_t* queries, void* hip_stream) {
    RAYRS_GUARDED({
    return lit_entry(scene, LitCall{LIT_START_RAY, samples, max_bounces, sample_chunk, 0.0, seed, index_base, fast_traversal, lights, n_lights, true},
                     origin, direction, n, radiance, queries, true, hip_stream);
    })
}

int rayrs_scene_irradiance_direct(rayrs_scene* scene, const double* position, const double* normal, uint64_t n, uint32_t samples,
                                  uint32_t max_bounces, uint32_t sample_chunk, double bias, uint64_t seed, uint64_t index_base,
                                  uint32_t fast_traversal, const uint32_t* lights, uint32_t n_lights, double* radiance, uint32_t* queries) {
    RAYRS_GUARDED({
    return lit_entry(scene, LitCall{LIT_START_POINT, samples, max_bounces, sample_chunk, bias, seed, index_base, fast_traversal, lights, n_lights, true},
                     position, normal, n, radiance, queries, false, nullptr);
    })
}

int rayrs_scene_irradiance_direct_launch(rayrs_scene* scene, const double* position, const double* normal, uint64_t n, uint32_t samples,
                                         uint32_t max_bounces, uint32_t sample_chunk, double bias, uint64_t seed, uint64_t index_base,
                                         uint32_t fast_traversal, const uint32_t* lights, uint32_t n_lights, double* radiance,
                                         uint32_t* queries, void* hip_stream) {
    RAYRS_GUARDED({
    return lit_entry(scene, LitCall{LIT_START_POINT, samples, max_bounces, sample_chunk, bias, seed, index_base, fast_traversal, lights, n_lights, true},
                     position, normal, n, radiance, queries, true, hip_stream);
    })
}

int rayrs_render_direct(rayrs_scene* scene, const rayrs_camera* camera, uint64_t seed, uint32_t samples, uint32_t max_bounces,
                        uint32_t sample_chunk, uint32_t fast_traversal, const uint32_t* lights, uint32_t n_lights, double* out_rgb,
                        uint32_t* queries) {
    RAYRS_GUARDED({
    return lit_render(scene, camera, LitCall{LIT_START_PIXEL, samples, max_bounces, sample_chunk, 0.0, seed, 0u, fast_traversal, lights, n_lights, true},
                      out_rgb, queries);
    })
}

}  // extern "C"
