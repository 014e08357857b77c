// denoise_kernels.h -- the film's per-pixel noise plane and the two a-trous filters (include/rayrs_hip.h DENOISER, NOISE
// PLANE and GUIDED FILTER; rayrs_film_denoise, rayrs_image_denoise, rayrs_film_noise, rayrs_film_denoise_guided,
// rayrs_image_denoise_guided): what denoise.hip's kernels are handed, and their launch wrappers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "layout.h"

namespace rayrs {

// One level of the feature-guided filter: out = the level's colour, from `color` and the read-only feature planes (each may
// be null: its term is left out).  kc is this level's kc * 4^level, formed by the host.
struct AtrousDev {
    const double* color;   // H * W * 3
    const double* normal;  // H * W * 3 or null
    const double* albedo;  // H * W * 3 or null
    const double* depth;   // H * W or null
    void* out;             // H * W * 3, f64, or f32 (the f64 result converted at the store) with out_f32
    uint32_t w, h;
    uint32_t step, out_f32;
    double kn, ka, kz, kc;
};

// The guided filter's working frame: one 32-byte record per pixel, row-major, so that a tap's colour and variance are one aligned
// 32-byte fetch and the 64 taps of a wave's row one 2 KB run.
struct GuidedRec {
    double cx, cy, cz, v;
};
static_assert(sizeof(GuidedRec) == 32, "GuidedRec");

// The noise plane of a film: variance (H * W, row-major, cleared to +0 by the caller) takes the pixels of the share's tiles.
struct FilmNoiseDev {
    const double* rec;       // the film's records (film.h)
    const uint32_t* tile_n;  // N_t per tile of the frame
    double* variance;
    uint32_t w, h;
    TileShare share;
    uint32_t c;
};

// One level of the variance-guided filter: reads the records of the level before and the read-only feature planes (each may be null: its
// term is left out).  A level that is not the last writes records; the last one stores the colour (f64, or f32 converted at
// the store) and, if wanted, the variance as planes.
struct GuidedDev {
    const GuidedRec* in;
    const double* normal;  // H * W * 3 or null
    const double* albedo;  // H * W * 3 or null
    const double* depth;   // H * W or null
    GuidedRec* out_rec;    // not the last level
    void* out_color;       // the last level: H * W * 3
    double* out_variance;  // the last level: H * W, or null
    uint32_t w, h;
    uint32_t step;
    uint32_t last, out_f32, pad;
    double kn, ka, kz, kv;
};

hipError_t launch_atrous(const AtrousDev& a, hipStream_t stream);
hipError_t launch_film_noise(const FilmNoiseDev& n, hipStream_t stream);
// records = (color, variance) per pixel: level 0's input
hipError_t launch_guided_pack(const double* color, const double* variance, GuidedRec* out, uint32_t w, uint32_t h, hipStream_t stream);
hipError_t launch_guided_atrous(const GuidedDev& g, hipStream_t stream);

}  // namespace rayrs
