// ao_kernels.h -- ambient occlusion (include/rayrs_hip.h AMBIENT OCCLUSION: rayrs_scene_ambient_occlusion, its _launch form
// and rayrs_render_ao): what ao.hip's kernels are handed, and their launch wrappers.
#pragma once
#include <hip/hip_runtime.h>

#include "layout.h"
#include "query_kernels.h"

namespace rayrs {

// A workgroup of ao_kernel owns a block of consecutive points and hands out their block_points x samples (point, sample)
// items to its four waves through a cursor in LDS; the points' counters live in LDS too.  About AO_BLOCK_ITEMS items a block
// (four a lane, so that a lane that finishes has something to take), at most AO_BLOCK_POINTS points (the counters).
constexpr uint32_t AO_BLOCK_POINTS = 256;
constexpr uint32_t AO_BLOCK_ITEMS = 1024;
// Refill a wave's idle lanes when fewer than this are walking, 1..64 (1: only when none walks).  32 is the best of the sweep
// over both point sets of profiles/ao_rates.txt: 19 % over no refill on rays that meet geometry (seven steps a ray), 3 % under
// it on rays that leave an open floor in under one step, where making a ray costs more than walking it.
constexpr uint32_t AO_REFILL_BELOW = 32;
constexpr uint32_t AO_LEAF_MIN = 24;      // run a leaf phase once this many lanes stand on a leaf group (the fast walk's setting)
inline uint32_t ao_block_points(uint32_t samples) {
    const uint32_t b = (AO_BLOCK_ITEMS + samples - 1u) / samples;  // (samples >= 1)
    return samples >= AO_BLOCK_ITEMS ? 1u : (b < AO_BLOCK_POINTS ? b : AO_BLOCK_POINTS);
}
// A launch's grid has at most QUERY_LAUNCH_RAYS threads (the stack strip is the queries'): the points one launch holds.
inline uint64_t ao_launch_points(uint32_t samples) { return QUERY_LAUNCH_RAYS / 256u * ao_block_points(samples); }

// One launch: the points 0 .. n - 1 behind these pointers (ao_abi.cpp moves them, and index_base, on from launch to launch).
struct AoDev {
    uint32_t n;
    uint32_t samples;
    uint32_t block_points;   // ao_block_points(samples)
    uint32_t refill_below;   // 1..64
    uint64_t seed, index_base;
    double t_max, bias;
    const double* position;  // n * 3
    const double* normal;    // n * 3
    const uint8_t* active;   // n, or null = every point; a point with 0 gets count 0 and no rays
    uint32_t* count;         // n, or null = not wanted
    double* visibility;      // n, or null = not wanted
    unsigned long long* turns;  // null, or two counters (the lab's instance): wave turns x 64, lane-turns spent walking
    uint32_t* spill;         // the traversal stacks' overflow: (stack_depth - stack_lds) words per thread of the grid
};

// The image form's first pass: the closest hit of sample 0's primary ray of every pixel, one lane per pixel, one wave per 8x8
// tile of the whole frame (tiles tile0 .. tile0 + n_tiles - 1 in this launch).  Writes, at pixel row * W + col: the hit's
// position, its normal turned against the ray, and active = 1; on a miss active = 0 (position and normal then hold zeros).
struct AoPrimaryDev {
    TileShare share;   // the whole frame: rank 0 of 1
    uint32_t tile0, n_tiles;
    uint64_t seed;
    double* position;  // H * W * 3
    double* normal;    // H * W * 3
    uint8_t* active;   // H * W
    uint32_t* spill;
};

inline uint64_t ao_threads(uint32_t n, uint32_t block_points) { return ((uint64_t)n + block_points - 1u) / block_points * 256u; }
hipError_t launch_ao(bool compact, const SceneDev& sc, const AoDev& ao, hipStream_t stream);
hipError_t launch_ao_primary(bool compact, const SceneDev& sc, const CameraDev& cam, const AoPrimaryDev& pd, hipStream_t stream);

}  // namespace rayrs
