// radiance_sky_abi.cpp -- the radiance queries with the sky among the lights of include/rayrs_hip.h (SKY SAMPLING): the table of the
// host scene's HDRI, its device copy, the three host-only calls over radiance_sky_table.h's functions, and the entry points.  The
// refusals, the light table, the launches and the host forms are the lit queries' (radiance_lit_abi.cpp), taken with
// LitCall::direct and LitCall::sky set.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/rayrs_hip.h"
#include "../../include/rayrs_numeric.h"
#include "radiance_lit_host.hpp"
#include "radiance_sky_table.h"

namespace rayrs {

// The table, once per scene: every step one f64 operation of the header's, in its order.  texel(i, j) is the clipped texel
// Scene::background reads: the first of the four that FlatScene::hdri_quads keeps for (i, j).
SkyDev sky_host_table(rayrs_scene* scene) {
    rayrs_scene::Sky& sky = scene->sky;
    const FlatScene& f = scene->flat;
    const uint32_t w = f.hdri_w, h = f.hdri_h;  // (both >= 2: build_flat_scene)
    if (!sky.built) {
        const uint32_t rows = h - 1u, cols = w - 1u;
        sky.table.assign(sky_table_doubles(w, h), 0.0);
        double* M = sky.table.data();
        double* C = M + rows;
        double* A = C + (size_t)rows * cols;
        auto L = [&](uint32_t i, uint32_t j) {
            const float* t = &f.hdri_quads[((size_t)i * w + j) * 16u];
            return ((double)t[0] + (double)t[1]) + (double)t[2];
        };
        for (uint32_t i = 0; i < rows; i++) {
            const double s_i = rr_sin(((double)i + 0.5) * RR_PI / (double)(h - 1u));
            for (uint32_t j = 0; j < cols; j++) {
                const double a = s_i * (((L(i, j) + L(i + 1u, j)) + L(i, j + 1u)) + L(i + 1u, j + 1u));
                A[(size_t)i * cols + j] = a;
                C[(size_t)i * cols + j] = j == 0u ? a : C[(size_t)i * cols + j - 1u] + a;
            }
            const double R_i = C[(size_t)i * cols + cols - 1u];
            M[i] = i == 0u ? R_i : M[i - 1u] + R_i;
        }
        sky.total = M[rows - 1u];
        sky.built = true;
    }
    return SkyDev{sky.table.data(), w, h, sky.total};
}

bool sky_table_usable(rayrs_scene* scene) {
    const double T = sky_host_table(scene).T;
    return T > 0.0 && std::isfinite(T);
}

int sky_device_table(rayrs_scene* scene, SkyDev* out) {
    SkyDev t = sky_host_table(scene);
    rayrs_scene::Sky& sky = scene->sky;
    if (!sky.uploaded) {
        HIP_TRY(sky.d_table.upload(sky.table.data(), sky.table.size() * sizeof(double)));
        sky.uploaded = true;
    }
    t.table = sky.d_table.as<const double>();
    *out = t;
    return RAYRS_OK;
}

}  // namespace rayrs

using namespace rayrs;

extern "C" {

int rayrs_scene_sky_table(rayrs_scene* scene, double* cells, double* total) {
    RAYRS_GUARDED({
    if (!scene || (!cells && !total)) return RAYRS_INVALID_ARG;
    const SkyDev t = sky_host_table(scene);
    if (cells) {
        const size_t n = (size_t)(t.h - 1u) * (t.w - 1u);
        const double* A = sky_A(t, 0u);
        for (size_t k = 0; k < n; k++) cells[k] = A[k];
    }
    if (total) *total = t.T;
    return RAYRS_OK;
    })
}

int rayrs_scene_sky_sample(rayrs_scene* scene, const double* u, uint64_t n, double* dir) {
    RAYRS_GUARDED({
    if (!scene || !u || !dir) return RAYRS_INVALID_ARG;
    if (!sky_table_usable(scene)) return RAYRS_UNSUPPORTED;
    const SkyDev t = sky_host_table(scene);
    for (uint64_t k = 0; k < n; k++) sky_sample(t, u[2u * k], u[2u * k + 1u], dir + 3u * k);
    return RAYRS_OK;
    })
}

int rayrs_scene_sky_density(rayrs_scene* scene, const double* dir, uint64_t n, double* p) {
    RAYRS_GUARDED({
    if (!scene || !dir || !p) return RAYRS_INVALID_ARG;
    if (!sky_table_usable(scene)) return RAYRS_UNSUPPORTED;
    const SkyDev t = sky_host_table(scene);
    for (uint64_t k = 0; k < n; k++) p[k] = sky_density(t, dir[3u * k], dir[3u * k + 1u], dir[3u * k + 2u]);
    return RAYRS_OK;
    })
}

int rayrs_scene_radiance_sky(rayrs_scene* scene, const double* origin, const double* direction, uint64_t n, uint32_t samples,
                             uint32_t max_bounces, uint32_t sample_chunk, uint64_t seed, uint64_t index_base, uint32_t fast_traversal,
                             const uint32_t* lights, uint32_t n_lights, double* radiance, uint32_t* queries) {
    RAYRS_GUARDED({
    return lit_entry(scene, LitCall{LIT_START_RAY, samples, max_bounces, sample_chunk, 0.0, seed, index_base, fast_traversal, lights, n_lights, true, true},
                     origin, direction, n, radiance, queries, false, nullptr);
    })
}

int rayrs_scene_radiance_sky_launch(rayrs_scene* scene, const double* origin, const double* direction, uint64_t n, uint32_t samples,
                                    uint32_t max_bounces, uint32_t sample_chunk, uint64_t seed, uint64_t index_base,
                                    uint32_t fast_traversal, const uint32_t* lights, uint32_t n_lights, double* radiance,
                                    uint32_t* queries, void* hip_stream) {
    RAYRS_GUARDED({
    return lit_entry(scene, LitCall{LIT_START_RAY, samples, max_bounces, sample_chunk, 0.0, seed, index_base, fast_traversal, lights, n_lights, true, true},
                     origin, direction, n, radiance, queries, true, hip_stream);
    })
}

int rayrs_scene_irradiance_sky(rayrs_scene* scene, const double* position, const double* normal, uint64_t n, uint32_t samples,
                               uint32_t max_bounces, uint32_t sample_chunk, double bias, uint64_t seed, uint64_t index_base,
                               uint32_t fast_traversal, const uint32_t* lights, uint32_t n_lights, double* radiance, uint32_t* queries) {
    RAYRS_GUARDED({
    return lit_entry(scene, LitCall{LIT_START_POINT, samples, max_bounces, sample_chunk, bias, seed, index_base, fast_traversal, lights, n_lights, true, true},
                     position, normal, n, radiance, queries, false, nullptr);
    })
}

int rayrs_scene_irradiance_sky_launch(rayrs_scene* scene, const double* position, const double* normal, uint64_t n, uint32_t samples,
                                      uint32_t max_bounces, uint32_t sample_chunk, double bias, uint64_t seed, uint64_t index_base,
                                      uint32_t fast_traversal, const uint32_t* lights, uint32_t n_lights, double* radiance,
                                      uint32_t* queries, void* hip_stream) {
    RAYRS_GUARDED({
    return lit_entry(scene, LitCall{LIT_START_POINT, samples, max_bounces, sample_chunk, bias, seed, index_base, fast_traversal, lights, n_lights, true, true},
                     position, normal, n, radiance, queries, true, hip_stream);
    })
}

int rayrs_render_sky(rayrs_scene* scene, const rayrs_camera* camera, uint64_t seed, uint32_t samples, uint32_t max_bounces,
                     uint32_t sample_chunk, uint32_t fast_traversal, const uint32_t* lights, uint32_t n_lights, double* out_rgb,
                     uint32_t* queries) {
    RAYRS_GUARDED({
    return lit_render(scene, camera, LitCall{LIT_START_PIXEL, samples, max_bounces, sample_chunk, 0.0, seed, 0u, fast_traversal, lights, n_lights, true, true},
                      out_rgb, queries);
    })
}

}  // extern "C"
