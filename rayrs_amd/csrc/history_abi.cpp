// history_abi.cpp -- temporal accumulation of include/rayrs_hip.h (rayrs_history_*, rayrs_camera_orbit): a history's
// lifetime, a push of the caller's planes or of a film's view through the reprojection kernel (temporal.hip), the
// history read back and put through the variance-guided filter (denoise_abi.cpp denoise_run).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "../../include/rayrs_hip.h"
#include "../../include/rayrs_numeric.h"
#include "denoise_host.hpp"
#include "film_host.hpp"
#include "scene_internal.hpp"
#include "temporal_kernels.h"

using namespace rayrs;

namespace {
// A view's planes on the device, in the form DenoiseIn wants them.
struct ViewPlanes {
    DevBuf color, variance, weight, normal, albedo, depth, coverage, object;
};
}  // namespace

struct rayrs_history {
    int device = -1;
    bool filled = false;
    rayrs_camera camera = {};   // of set[cur], once filled
    bool has_albedo = false;    // ... rayrs_history_push_image may leave it out
    // Two sets, ping-ponged: a push reads set[cur] as B and writes set[cur ^ 1], A's features and the blend.
    ViewPlanes set[2];
    int cur = 0;
    DevBuf in_color, in_variance, in_weight;  // rayrs_history_push_image: the incoming frame
    DevBuf d_prim_object;                     // rayrs_history_push_film: depth-first slot -> object of the film's scene
    DenoiseBufs filter;                       // what rayrs_history_denoise_guided works in
    Event ev[6];                              // rayrs_history_push_film: around features, frame, noise, copies, reprojection
    bool has_events = false, timed = false;
};

// the scalars' refusals, which every push shares
static int push_check(double max_weight, double depth_tol, double normal_tol) {
    if (!(max_weight > 0.0) || !std::isfinite(max_weight)) return RAYRS_INVALID_ARG;
    for (const double tol : {depth_tol, normal_tol})
        if (!(tol >= 0.0) || !std::isfinite(tol)) return RAYRS_INVALID_ARG;
    return RAYRS_OK;
}

// Sizes the set a push writes for a view of npix pixels.
static int reserve_view(ViewPlanes& v, size_t npix) {
    HIP_TRY(v.color.reserve(npix * 3 * sizeof(double)));
    HIP_TRY(v.variance.reserve(npix * sizeof(double)));
    HIP_TRY(v.weight.reserve(npix * sizeof(double)));
    HIP_TRY(v.normal.reserve(npix * 3 * sizeof(double)));
    HIP_TRY(v.albedo.reserve(npix * 3 * sizeof(double)));
    HIP_TRY(v.depth.reserve(npix * sizeof(double)));
    HIP_TRY(v.coverage.reserve(npix * sizeof(double)));
    HIP_TRY(v.object.reserve(npix * sizeof(uint32_t)));
    return RAYRS_OK;
}

// The kernel's arguments but A's colour, variance, weight and object source: B is set[cur], the output and A's features
// set[cur ^ 1] (already filled in).
static TemporalDev push_args(const rayrs_history* h, const rayrs_camera* cam, double max_weight, double depth_tol, double normal_tol) {
    const ViewPlanes& a = h->set[h->cur ^ 1];
    const ViewPlanes& b = h->set[h->cur];
    TemporalDev t;
    std::memset(&t, 0, sizeof(t));
    t.cam_a = make_camera_dev(cam);
    t.cam_b = make_camera_dev(h->filled ? &h->camera : cam);
    t.a_normal = a.normal.as<double>(), t.a_depth = a.depth.as<double>(), t.a_coverage = a.coverage.as<double>();
    t.a_object = a.object.as<uint32_t>();
    t.has_b = h->filled ? 1u : 0u;
    t.b_color = b.color.as<double>(), t.b_variance = b.variance.as<double>(), t.b_weight = b.weight.as<double>();
    t.b_normal = b.normal.as<double>(), t.b_depth = b.depth.as<double>(), t.b_coverage = b.coverage.as<double>();
    t.b_object = b.object.as<uint32_t>();
    t.max_weight = max_weight, t.tz2 = depth_tol * depth_tol, t.tn2 = normal_tol * normal_tol;
    t.out_color = a.color.as<double>(), t.out_variance = a.variance.as<double>(), t.out_weight = a.weight.as<double>();
    return t;
}

static void push_done(rayrs_history* h, const rayrs_camera* cam, bool has_albedo) {
    h->cur ^= 1;
    h->camera = *cam;
    h->has_albedo = has_albedo;
    h->filled = true;
}

extern "C" {

int rayrs_history_create(int device, rayrs_history** out) {
    RAYRS_GUARDED({
    if (!out) return RAYRS_INVALID_ARG;
    *out = new rayrs_history();
    (*out)->device = device;  // the device is first touched by a push
    return RAYRS_OK;
    })
}

void rayrs_history_destroy(rayrs_history* h) {
    if (!h) return;
    if (h->device >= 0 && (h->filled || h->has_events)) (void)hipSetDevice(h->device);
    delete h;
}

int rayrs_history_reset(rayrs_history* h) {
    if (!h) return RAYRS_INVALID_ARG;
    h->filled = false, h->timed = false;  // the buffers are kept for the next push
    return RAYRS_OK;
}

int rayrs_history_push_image(rayrs_history* h, const rayrs_camera* camera, const double* color, const double* variance,
                             const double* weight, const double* normal, const double* albedo, const double* depth,
                             const double* coverage, const uint32_t* object, double max_weight, double depth_tol, double normal_tol) {
    RAYRS_GUARDED({
    if (!h || !color || !variance || !weight || !normal || !depth || !coverage || !object) return RAYRS_INVALID_ARG;
    if (!camera || camera->x_pixels == 0u || camera->y_pixels == 0u) return RAYRS_INVALID_ARG;
    RAYRS_TRY(push_check(max_weight, depth_tol, normal_tol));
    if (camera->x_pixels > 65535u || camera->y_pixels > 65535u) return RAYRS_UNSUPPORTED;
    if (h->device < 0) return RAYRS_NO_DEVICE;
    HIP_TRY(hipSetDevice(h->device));
    const size_t npix = (size_t)camera->x_pixels * camera->y_pixels;
    ViewPlanes& a = h->set[h->cur ^ 1];
    RAYRS_TRY(reserve_view(a, npix));
    HIP_TRY(h->in_color.upload(color, npix * 3 * sizeof(double)));
    HIP_TRY(h->in_variance.upload(variance, npix * sizeof(double)));
    HIP_TRY(h->in_weight.upload(weight, npix * sizeof(double)));
    HIP_TRY(a.normal.upload(normal, npix * 3 * sizeof(double)));
    if (albedo) HIP_TRY(a.albedo.upload(albedo, npix * 3 * sizeof(double)));
    HIP_TRY(a.depth.upload(depth, npix * sizeof(double)));
    HIP_TRY(a.coverage.upload(coverage, npix * sizeof(double)));
    HIP_TRY(a.object.upload(object, npix * sizeof(uint32_t)));
    TemporalDev t = push_args(h, camera, max_weight, depth_tol, normal_tol);
    t.a_color = h->in_color.as<double>(), t.a_variance = h->in_variance.as<double>(), t.a_weight = h->in_weight.as<double>();
    HIP_TRY(launch_temporal(t, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    h->timed = false;
    push_done(h, camera, albedo != nullptr);
    return RAYRS_OK;
    })
}

int rayrs_history_push_film(rayrs_history* h, rayrs_film* film, uint32_t feature_samples, double max_weight, double depth_tol,
                            double normal_tol) {
    RAYRS_GUARDED({
    if (!h || !film) return RAYRS_INVALID_ARG;
    int film_device = -1;
    RAYRS_TRY(film_view_check(film, feature_samples, &film_device));
    RAYRS_TRY(push_check(max_weight, depth_tol, normal_tol));
    if (film_device != h->device) return RAYRS_INVALID_ARG;
    if (h->device < 0) return RAYRS_NO_DEVICE;
    HIP_TRY(hipSetDevice(h->device));
    if (!h->has_events) {
        for (Event& e : h->ev) HIP_TRY(e.create());
        h->has_events = true;
    }
    h->timed = false;
    FilmView v;
    HIP_TRY(hipEventRecord(h->ev[0], nullptr));
    const hipEvent_t marks[3] = {h->ev[1], h->ev[2], h->ev[3]};  // behind the features, the frame, the noise plane
    RAYRS_TRY(film_view(film, feature_samples, &v, marks));
    const rayrs_camera* camera = v.camera;
    const size_t npix = (size_t)camera->x_pixels * camera->y_pixels;
    ViewPlanes& a = h->set[h->cur ^ 1];
    RAYRS_TRY(reserve_view(a, npix));
    // the history keeps its own copy of the view's features: the film may make others, or go away
    HIP_TRY(hipMemcpyAsync(a.normal.as<>(), v.normal, npix * 3 * sizeof(double), hipMemcpyDeviceToDevice, nullptr));
    HIP_TRY(hipMemcpyAsync(a.albedo.as<>(), v.albedo, npix * 3 * sizeof(double), hipMemcpyDeviceToDevice, nullptr));
    HIP_TRY(hipMemcpyAsync(a.depth.as<>(), v.depth, npix * sizeof(double), hipMemcpyDeviceToDevice, nullptr));
    HIP_TRY(hipMemcpyAsync(a.coverage.as<>(), v.coverage, npix * sizeof(double), hipMemcpyDeviceToDevice, nullptr));
    const std::vector<uint32_t>& prim_object = v.scene->flat.prim_object;
    HIP_TRY(h->d_prim_object.reserve((prim_object.size() + 1u) * sizeof(uint32_t)));
    if (!prim_object.empty())
        HIP_TRY(hipMemcpyAsync(h->d_prim_object.as<>(), prim_object.data(), prim_object.size() * sizeof(uint32_t), hipMemcpyHostToDevice, nullptr));
    HIP_TRY(hipEventRecord(h->ev[4], nullptr));
    TemporalDev t = push_args(h, camera, max_weight, depth_tol, normal_tol);
    t.a_color = v.color, t.a_variance = v.variance;
    t.a_weight = nullptr, t.a_tile_n = v.tile_n, t.a_tiles_x = v.tiles_x;
    t.a_object = v.prim;
    t.prim_object = h->d_prim_object.as<uint32_t>(), t.n_prims = (uint32_t)prim_object.size();
    t.out_object = a.object.as<uint32_t>();
    HIP_TRY(launch_temporal(t, nullptr));
    HIP_TRY(hipEventRecord(h->ev[5], nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));  // (prim_object is the scene's own vector: the copy from it has ended)
    h->timed = true;
    push_done(h, camera, true);
    return RAYRS_OK;
    })
}

int rayrs_history_push_times(rayrs_history* h, double ms[5]) {
    RAYRS_GUARDED({
    if (!h || !ms || !h->timed) return RAYRS_INVALID_ARG;
    HIP_TRY(hipSetDevice(h->device));
    for (int k = 0; k < 5; k++) {
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, h->ev[k], h->ev[k + 1]));
        ms[k] = (double)t;
    }
    return RAYRS_OK;
    })
}

int rayrs_history_read(rayrs_history* h, uint32_t out_format, void* color, void* variance, void* weight) {
    RAYRS_GUARDED({
    if (!h || !h->filled) return RAYRS_INVALID_ARG;
    if (out_format != RAYRS_OUT_F32 && out_format != RAYRS_OUT_F64) return RAYRS_INVALID_ARG;
    if (h->device < 0) return RAYRS_NO_DEVICE;
    HIP_TRY(hipSetDevice(h->device));
    const size_t npix = (size_t)h->camera.x_pixels * h->camera.y_pixels;
    const ViewPlanes& s = h->set[h->cur];
    std::vector<double> stage;
    // RAYRS_OUT_F32 is the f64 plane converted element by element, as image.rs:224-229 converts a frame
    auto fetch = [&](const DevBuf& src, size_t n, void* dst) -> hipError_t {
        if (out_format == RAYRS_OUT_F64) return src.download(dst, n * sizeof(double));
        stage.resize(n);
        const hipError_t e = src.download(stage.data(), n * sizeof(double));
        if (e == hipSuccess)
            for (size_t k = 0; k < n; k++) static_cast<float*>(dst)[k] = (float)stage[k];
        return e;
    };
    if (color) HIP_TRY(fetch(s.color, npix * 3, color));
    if (variance) HIP_TRY(fetch(s.variance, npix, variance));
    if (weight) HIP_TRY(fetch(s.weight, npix, weight));
    return RAYRS_OK;
    })
}

int rayrs_history_denoise_guided(rayrs_history* h, uint32_t levels, double kn, double ka, double kz, double kv, uint32_t out_format,
                                 void* out_host, double* out_variance) {
    RAYRS_GUARDED({
    if (!h || !out_host || !h->filled) return RAYRS_INVALID_ARG;
    if (out_format != RAYRS_OUT_F32 && out_format != RAYRS_OUT_F64) return RAYRS_INVALID_ARG;
    RAYRS_TRY(denoise_check(levels, kn, ka, kz, kv));
    if (h->device < 0) return RAYRS_NO_DEVICE;
    HIP_TRY(hipSetDevice(h->device));
    const uint32_t w = h->camera.x_pixels, hh = h->camera.y_pixels;
    const ViewPlanes& s = h->set[h->cur];
    const DenoiseIn in{w, hh, s.color.as<double>(), s.variance.as<double>(), s.normal.as<double>(),
                       h->has_albedo ? s.albedo.as<double>() : nullptr, s.depth.as<double>()};
    const void* result = nullptr;
    RAYRS_TRY(denoise_run(in, levels, kn, ka, kz, kv, out_format, out_variance != nullptr, h->filter, &result));
    HIP_TRY(hipMemcpy(out_host, result, frame_bytes(w, hh, out_format), hipMemcpyDeviceToHost));
    if (out_variance) HIP_TRY(h->filter.variance.download(out_variance, (size_t)w * hh * sizeof(double)));
    return RAYRS_OK;
    })
}

int rayrs_camera_orbit(const double origin[3], const double up[3], const double lookat[3], double degrees, double out_origin[3]) {
    if (!origin || !up || !lookat || !out_origin || !std::isfinite(degrees)) return RAYRS_INVALID_ARG;
    const double n2 = (up[0] * up[0] + up[1] * up[1]) + up[2] * up[2];
    if (!(n2 > 0.0) || !std::isfinite(n2)) return RAYRS_INVALID_ARG;
    if (degrees == 0.0) {  // the origin itself, not lookat + (origin - lookat)
        for (int i = 0; i < 3; i++) out_origin[i] = origin[i];
        return RAYRS_OK;
    }
    const double inv = 1.0 / rr_sqrt(n2);
    const double k[3] = {up[0] * inv, up[1] * inv, up[2] * inv};
    const double v[3] = {origin[0] - lookat[0], origin[1] - lookat[1], origin[2] - lookat[2]};
    const double rad = degrees * (RR_PI / 180.0);
    const double c = rr_cos(rad), s = rr_sin(rad);
    const double kv = (k[0] * v[0] + k[1] * v[1]) + k[2] * v[2];
    const double g = kv * (1.0 - c);
    const double x[3] = {k[1] * v[2] - k[2] * v[1], k[2] * v[0] - k[0] * v[2], k[0] * v[1] - k[1] * v[0]};
    for (int i = 0; i < 3; i++) out_origin[i] = lookat[i] + ((v[i] * c + x[i] * s) + k[i] * g);
    return RAYRS_OK;
}

}  // extern "C"
