// denoise_abi.cpp -- the two a-trous filters of include/rayrs_hip.h on frames of the caller's (rayrs_image_denoise,
// rayrs_image_denoise_guided) and what film_abi.cpp's rayrs_film_denoise / rayrs_film_denoise_guided share with them: the
// refusals and the filter's levels (denoise.hip).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "../../include/rayrs_hip.h"
#include "denoise_host.hpp"
#include "scene_internal.hpp"

using namespace rayrs;

namespace rayrs {

int denoise_check(uint32_t levels, double kn, double ka, double kz, double k) {
    if (levels < 1u || levels > 16u) return RAYRS_INVALID_ARG;
    for (const double v : {kn, ka, kz, k})
        if (!(v >= 0.0) || !std::isfinite(v)) return RAYRS_INVALID_ARG;
    return RAYRS_OK;
}

int denoise_run(const DenoiseIn& in, uint32_t levels, double kn, double ka, double kz, double k, uint32_t out_format,
                bool want_variance, DenoiseBufs& b, const void** result) {
    const bool guided = in.variance != nullptr;
    const size_t npix = (size_t)in.w * in.h;
    const size_t bytes = npix * (guided ? sizeof(GuidedRec) : 3 * sizeof(double));
    // level 0 writes frame[0]; the guided filter reads its packed records from frame[1] there, the plain one in.color
    HIP_TRY(b.frame[guided ? 1 : 0].reserve(bytes));
    if (levels > 1u) HIP_TRY(b.frame[guided ? 0 : 1].reserve(bytes));
    AtrousDev a;
    GuidedDev g;
    std::memset(&a, 0, sizeof(a));
    std::memset(&g, 0, sizeof(g));
    a.normal = g.normal = in.normal, a.albedo = g.albedo = in.albedo, a.depth = g.depth = in.depth;
    a.w = g.w = in.w, a.h = g.h = in.h;
    a.kn = g.kn = kn, a.ka = g.ka = ka, a.kz = g.kz = kz, g.kv = k;
    if (guided) {
        HIP_TRY(b.color.reserve(npix * 3 * sizeof(double)));
        if (want_variance) HIP_TRY(b.variance.reserve(npix * sizeof(double)));
        HIP_TRY(launch_guided_pack(in.color, in.variance, b.frame[1].as<GuidedRec>(), in.w, in.h, nullptr));
    }
    double kc_k = k;  // kc * 4^level: a power of two times kc, the same bits however it is formed
    for (uint32_t level = 0; level < levels; level++) {
        const DevBuf& src = b.frame[(level & 1u) ^ 1u];
        const DevBuf& dst = b.frame[level & 1u];
        const bool last = level + 1u == levels;
        const uint32_t out_f32 = last && out_format == RAYRS_OUT_F32 ? 1u : 0u;
        if (guided) {
            g.in = src.as<GuidedRec>();
            g.step = 1u << level;
            g.last = last ? 1u : 0u;
            g.out_rec = last ? nullptr : dst.as<GuidedRec>();
            g.out_color = last ? b.color.as<>() : nullptr;
            g.out_variance = last && want_variance ? b.variance.as<double>() : nullptr;
            g.out_f32 = out_f32;
            HIP_TRY(launch_guided_atrous(g, nullptr));
        } else {
            a.color = level ? src.as<double>() : in.color;
            a.out = dst.as<>();
            a.step = 1u << level;
            a.kc = kc_k;
            a.out_f32 = out_f32;
            HIP_TRY(launch_atrous(a, nullptr));
            kc_k *= 4.0;
        }
    }
    *result = guided ? b.color.as<>() : b.frame[(levels - 1u) & 1u].as<>();
    return RAYRS_OK;
}

}  // namespace rayrs

// Both rayrs_image_* calls: the refusals, the caller's planes uploaded to `device`, the levels, the result copied back.
// guided: `variance` is wanted too, k is kv and out_variance may be asked for.
static int image_denoise(int device, uint32_t w, uint32_t h, const double* color, const double* variance, bool guided,
                         const double* normal, const double* albedo, const double* depth, uint32_t levels, double kn, double ka,
                         double kz, double k, double* out, double* out_variance) {
    if (!color || (guided && !variance) || !out || w == 0u || h == 0u) return RAYRS_INVALID_ARG;
    RAYRS_TRY(denoise_check(levels, kn, ka, kz, k));  // the same rule for kv as for kc
    if (w > 65535u || h > 65535u) return RAYRS_UNSUPPORTED;
    if (device < 0) return RAYRS_NO_DEVICE;
    HIP_TRY(hipSetDevice(device));
    const size_t npix = (size_t)w * h;
    DevBuf d_color, d_variance, d_normal, d_albedo, d_depth;
    DenoiseBufs b;
    HIP_TRY(d_color.upload(color, npix * 3 * sizeof(double)));
    if (guided) HIP_TRY(d_variance.upload(variance, npix * sizeof(double)));
    if (normal) HIP_TRY(d_normal.upload(normal, npix * 3 * sizeof(double)));
    if (albedo) HIP_TRY(d_albedo.upload(albedo, npix * 3 * sizeof(double)));
    if (depth) HIP_TRY(d_depth.upload(depth, npix * sizeof(double)));
    const DenoiseIn in{w, h, d_color.as<double>(), d_variance.as<double>(), d_normal.as<double>(), d_albedo.as<double>(),
                       d_depth.as<double>()};
    const void* result = nullptr;
    RAYRS_TRY(denoise_run(in, levels, kn, ka, kz, k, RAYRS_OUT_F64, out_variance != nullptr, b, &result));
    HIP_TRY(hipMemcpy(out, result, frame_bytes(w, h, RAYRS_OUT_F64), hipMemcpyDeviceToHost));
    if (out_variance) HIP_TRY(b.variance.download(out_variance, npix * sizeof(double)));
    return RAYRS_OK;
}

extern "C" {

int rayrs_image_denoise(int device, uint32_t w, uint32_t h, const double* color, const double* normal, const double* albedo,
                        const double* depth, uint32_t levels, double kn, double ka, double kz, double kc, double* out) {
    RAYRS_GUARDED({ return image_denoise(device, w, h, color, nullptr, false, normal, albedo, depth, levels, kn, ka, kz, kc, out, nullptr); })
}

int rayrs_image_denoise_guided(int device, uint32_t w, uint32_t h, const double* color, const double* variance, const double* normal,
                               const double* albedo, const double* depth, uint32_t levels, double kn, double ka, double kz, double kv,
                               double* out, double* out_variance) {
    RAYRS_GUARDED({ return image_denoise(device, w, h, color, variance, true, normal, albedo, depth, levels, kn, ka, kz, kv, out, out_variance); })
}

}  // extern "C"
