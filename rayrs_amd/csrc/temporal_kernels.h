// temporal_kernels.h -- temporal accumulation (include/rayrs_hip.h TEMPORAL ACCUMULATION; rayrs_history_push_image,
// rayrs_history_push_film): what temporal.hip's reprojection kernel is handed, and its launch wrapper.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "layout.h"

namespace rayrs {

// One push: the incoming view A is blended into `out_*` with what the history B holds where A's first hits are seen from B.
// Every plane is row-major in its own view's size; colours and normals are 3 doubles per pixel.
struct TemporalDev {
    CameraDev cam_a, cam_b;  // wave-uniform: both are kernel arguments
    // A: the incoming frame
    const double* a_color;
    const double* a_variance;
    const double* a_weight;    // H * W, or null: the weight is (double)a_tile_n[tile of the pixel], a film's N_t
    const uint32_t* a_tile_n;  // one word per 8x8 tile, a_tiles_x tiles in a row
    const double* a_normal;
    const double* a_depth;
    const double* a_coverage;
    const uint32_t* a_object;  // object numbers, or, with prim_object, a features pass's depth-first slots
    // null, or n_prims words: depth-first slot -> object in insertion order (0xffffffff stays); the object numbers are then
    // also WRITTEN to out_object, the history's own object plane
    const uint32_t* prim_object;
    uint32_t* out_object;
    uint32_t n_prims, a_tiles_x;
    // B: the history; has_b = 0: it is empty, and every pixel that is not passed through has no history
    const double* b_color;
    const double* b_variance;
    const double* b_weight;
    const double* b_normal;
    const double* b_depth;
    const double* b_coverage;
    const uint32_t* b_object;
    uint32_t has_b, pad;
    double max_weight, tz2, tn2;
    // the history after the push, in A's size
    double* out_color;
    double* out_variance;
    double* out_weight;
};

hipError_t launch_temporal(const TemporalDev& t, hipStream_t stream);

}  // namespace rayrs
