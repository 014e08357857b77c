// feature_kernels.h -- first-hit feature buffers and the feature-guided a-trous filter (include/rayrs_hip.h
// rayrs_render_features, rayrs_film_features, rayrs_film_denoise, rayrs_image_denoise): what features.hip's two kernels
// are handed, and their launch wrappers.  (Not "features.h": a header of that name in this directory would stand in for the C
// library's own <features.h> wherever the directory is on the include path.)
#pragma once
#include <hip/hip_runtime.h>

#include "layout.h"

namespace rayrs {

// A features pass: the first hit of the samples 0 .. samples - 1 of every pixel of a tile share, summed per pixel in
// sample order.  All five planes are written, in image order (row-major, origin upper left); pixels outside the share
// are not touched (the caller clears the planes first).
struct FeatureDev {
    uint32_t samples;
    uint32_t tile_rank, tile_ranks;
    uint32_t tiles_x, n_local_tiles, pad;
    uint64_t seed;
    double inv_samples;  // 1.0 / (double)samples
    double* normal;      // H * W * 3
    double* albedo;      // H * W * 3
    double* depth;       // H * W
    double* coverage;    // H * W
    uint32_t* prim;      // H * W: the depth-first slot of the primitive sample 0 hit, 0xffffffff = none
    uint32_t* spill;     // the traversal stacks' overflow: (stack_depth - stack_lds) words per thread of the grid
};

// One level of the filter: out = the level's colour, from `color` and the read-only feature planes (each may be null: its
// term is left out).  kc is this level's kc * 4^level, formed by the host.
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

// threads of the features grid (whole workgroups of four waves, one wave per tile of the share): sizes the spill strip
inline uint64_t features_threads(uint32_t n_local_tiles) { return ((uint64_t)n_local_tiles + 3u) / 4u * 256u; }
hipError_t launch_features(bool compact, const SceneDev& sc, const CameraDev& cam, const FeatureDev& fd, hipStream_t stream);
hipError_t launch_atrous(const AtrousDev& a, hipStream_t stream);

}  // namespace rayrs
