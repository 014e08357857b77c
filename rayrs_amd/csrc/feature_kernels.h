// feature_kernels.h -- first-hit feature buffers (include/rayrs_hip.h rayrs_render_features, rayrs_film_features): what
// features.hip's kernel is handed, and its launch wrapper.  (Not "features.h": a header of that name in this directory would stand in for the C
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
    TileShare share;
    uint64_t seed;
    double inv_samples;  // 1.0 / (double)samples
    double* normal;      // H * W * 3
    double* albedo;      // H * W * 3
    double* depth;       // H * W
    double* coverage;    // H * W
    uint32_t* prim;      // H * W: the depth-first slot of the primitive sample 0 hit, 0xffffffff = none
    uint32_t* spill;     // the traversal stacks' overflow: (stack_depth - stack_lds) words per thread of the grid
};

// threads of the features grid (whole workgroups of four waves, one wave per tile of the share): sizes the spill strip
inline uint64_t features_threads(uint32_t n_local_tiles) { return ((uint64_t)n_local_tiles + 3u) / 4u * 256u; }
hipError_t launch_features(bool compact, const SceneDev& sc, const CameraDev& cam, const FeatureDev& fd, hipStream_t stream);

}  // namespace rayrs
