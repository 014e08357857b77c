// guided_abi.cpp -- the variance-guided a-trous filter of include/rayrs_hip.h (rayrs_image_denoise_guided) and what
// film_abi.cpp's rayrs_film_denoise_guided shares with it: the filter's levels (guided.hip).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "../../include/rayrs_hip.h"
#include "features_host.hpp"

using namespace rayrs;

namespace rayrs {

int guided_run(uint32_t w, uint32_t h, const double* d_color, const double* d_variance, const double* d_normal, const double* d_albedo,
               const double* d_depth, uint32_t levels, double kn, double ka, double kz, double kv, uint32_t out_format,
               bool want_variance, GuidedBufs& b) {
    const size_t npix = (size_t)w * h;
    HIP_TRY(b.ping.reserve(npix * sizeof(GuidedRec)));
    if (levels > 1u) HIP_TRY(b.pong.reserve(npix * sizeof(GuidedRec)));
    HIP_TRY(b.color.reserve(npix * 3 * sizeof(double)));
    if (want_variance) HIP_TRY(b.variance.reserve(npix * sizeof(double)));
    HIP_TRY(launch_guided_pack(d_color, d_variance, b.ping.as<GuidedRec>(), w, h, nullptr));
    GuidedDev g;
    std::memset(&g, 0, sizeof(g));
    g.normal = d_normal, g.albedo = d_albedo, g.depth = d_depth;
    g.w = w, g.h = h;
    g.kn = kn, g.ka = ka, g.kz = kz, g.kv = kv;
    for (uint32_t level = 0; level < levels; level++) {
        DevBuf& src = (level & 1u) ? b.pong : b.ping;
        DevBuf& dst = (level & 1u) ? b.ping : b.pong;
        g.in = src.as<GuidedRec>();
        g.step = 1u << level;
        g.last = level + 1u == levels ? 1u : 0u;
        if (g.last) {
            g.out_rec = nullptr;
            g.out_color = b.color.as<>();
            g.out_variance = want_variance ? b.variance.as<double>() : nullptr;
            g.out_f32 = out_format == RAYRS_OUT_F32 ? 1u : 0u;
        } else {
            g.out_rec = dst.as<GuidedRec>();
        }
        HIP_TRY(launch_guided_atrous(g, nullptr));
    }
    return RAYRS_OK;
}

}  // namespace rayrs

extern "C" {

int rayrs_image_denoise_guided(int device, uint32_t w, uint32_t h, const double* color, const double* variance, const double* normal,
                               const double* albedo, const double* depth, uint32_t levels, double kn, double ka, double kz, double kv,
                               double* out, double* out_variance) {
    RAYRS_GUARDED({
    if (!color || !variance || !out || w == 0u || h == 0u) return RAYRS_INVALID_ARG;
    RAYRS_TRY(denoise_check(levels, kn, ka, kz, kv));  // the same rule for kv as for kc
    if (w > 65535u || h > 65535u) return RAYRS_UNSUPPORTED;
    if (device < 0) return RAYRS_NO_DEVICE;
    HIP_TRY(hipSetDevice(device));
    const size_t npix = (size_t)w * h;
    DevBuf d_color, d_variance, d_normal, d_albedo, d_depth;
    GuidedBufs b;
    HIP_TRY(d_color.upload(color, npix * 3 * sizeof(double)));
    HIP_TRY(d_variance.upload(variance, npix * sizeof(double)));
    if (normal) HIP_TRY(d_normal.upload(normal, npix * 3 * sizeof(double)));
    if (albedo) HIP_TRY(d_albedo.upload(albedo, npix * 3 * sizeof(double)));
    if (depth) HIP_TRY(d_depth.upload(depth, npix * sizeof(double)));
    RAYRS_TRY(guided_run(w, h, d_color.as<double>(), d_variance.as<double>(), d_normal.as<double>(), d_albedo.as<double>(),
                         d_depth.as<double>(), levels, kn, ka, kz, kv, RAYRS_OUT_F64, out_variance != nullptr, b));
    HIP_TRY(b.color.download(out, npix * 3 * sizeof(double)));
    if (out_variance) HIP_TRY(b.variance.download(out_variance, npix * sizeof(double)));
    return RAYRS_OK;
    })
}

}  // extern "C"
