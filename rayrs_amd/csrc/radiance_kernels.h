// radiance_kernels.h -- radiance queries (include/rayrs_hip.h RADIANCE QUERY, IRRADIANCE: rayrs_scene_radiance,
// rayrs_scene_irradiance and their _launch forms): what radiance.hip's kernels are handed, and their launch wrappers.
#pragma once
#include <hip/hip_runtime.h>

#include "layout.h"
#include "query_kernels.h"

namespace rayrs {

// An item is (ray, chunk): the samples chunk * c' .. of one ray, summed in one lane in sample order.  A launch takes whole
// rays, at most RADIANCE_LAUNCH_ITEMS items, and hands them out from ONE cursor in device memory to a grid sized to the
// device: a lone probe's thousand chunks spread over as many waves as there are, not over one workgroup.
constexpr uint64_t RADIANCE_LAUNCH_ITEMS = 1ull << 20;
// Workgroups per CU of radiance_kernel's grid: two waves per SIMD is what its registers allow.
constexpr uint32_t RADIANCE_BLOCKS_PER_CU = 2;
// The wave's thresholds, 1..64 each (rayrs_lab.h rayrs_lab_radiance_tuning), each the best geometric mean of its sweep over
// both sets and both walks of profiles/radiance_rates.txt (headline scene).  On those sets a path makes 1.0 to 1.3
// queries, and the cheapest schedule is the plainest: finished lanes wait until no lane of the wave walks, are shaded together,
// and the lanes whose items ended are refilled in that same turn (22 to 26 % over 32 / 32 / 32 on the irradiance set, 8 to 10 % on
// the radiance set).  On rays that meet the mesh first it is the other way round by 0 to 15 % (the file's off_floor sets).
constexpr uint32_t RADIANCE_REFILL_BELOW = 1;   // idle lanes take new items when fewer than this many lanes are walking
constexpr uint32_t RADIANCE_SHADE_AT = 64;      // finished lanes are shaded once there are this many (or none walks)
constexpr uint32_t RADIANCE_LEAF_MIN = 1;       // run a leaf phase once this many lanes stand on a leaf group (flat on the chosen sets, best off the floor)

// The scene's scratch for one launch: the cursor, then 24 bytes (a chunk's sum) and 4 bytes (its query count) per item.
constexpr size_t RADIANCE_CURSOR_BYTES = 16;
constexpr size_t RADIANCE_SCRATCH_BYTES = RADIANCE_CURSOR_BYTES + RADIANCE_LAUNCH_ITEMS * (24u + 4u);

// One launch: the rays (points) 0 .. n - 1 behind these pointers (radiance_abi.cpp moves them, and index_base, on from
// launch to launch).
struct RadianceDev {
    uint32_t n;
    uint32_t samples;       // S
    uint32_t chunk;         // c': samples per chunk, 1..S
    uint32_t chunks;        // chunks per ray: ceil(S / c'); n * chunks <= RADIANCE_LAUNCH_ITEMS
    uint32_t max_bounces;   // >= 1 (0 never reaches a kernel: the answer is zeros)
    uint32_t irradiance;    // 0: a is origins, b directions; 1: a is points, b normals, and a sample's ray is made on draws 0 and 1
    uint32_t refill_below, shade_at, leaf_min;  // 1..64
    uint64_t seed, index_base;
    double bias;
    const double* a;        // n * 3
    const double* b;        // n * 3
    unsigned long long* cursor;  // zero at the launch
    double* partial;        // the items' sums, 3 per item, item = ray * chunks + chunk
    uint32_t* partial_queries;   // the items' query counts
    double* radiance;       // n * 3, or null = not wanted
    uint32_t* queries;      // n, or null = not wanted
    unsigned long long* turns;  // null, or three counters (the lab's instance): wave turns x 64, lane-turns spent walking, shading
    uint32_t* spill;        // the traversal stacks' overflow: (stack_depth - stack_lds) words per thread of the grid
};

// samples per chunk and chunks per ray of a call (rayrs_render_params.sample_chunk's rule)
inline uint32_t radiance_chunk(uint32_t samples, uint32_t sample_chunk) {
    return sample_chunk == 0u || sample_chunk >= samples ? samples : sample_chunk;
}
inline uint32_t radiance_chunks(uint32_t samples, uint32_t sample_chunk) {
    const uint32_t c = radiance_chunk(samples, sample_chunk);
    return (samples + c - 1u) / c;  // (samples + c - 1 < 2^31: samples < 2^30)
}

// The grid of every kernel that runs the radiance wave over rd's items (radiance.hip, radiance_lit.hip, radiance_direct.hip,
// radiance_sky.hip, film_direct.hip, bake.hip): cu_count * RADIANCE_BLOCKS_PER_CU workgroups, at most the queries' stack strip's
// and at most a wave per 64 items.
inline uint32_t radiance_grid_blocks(const RadianceDev& rd, int cu_count) {
    const uint64_t n_items = (uint64_t)rd.n * rd.chunks;
    const uint64_t waves = (n_items + 63u) / 64u;  // (a wave takes up to 64 items at its first refill)
    uint64_t blocks = (uint64_t)(cu_count > 0 ? cu_count : 1) * RADIANCE_BLOCKS_PER_CU;
    if (blocks > QUERY_LAUNCH_RAYS / 256u) blocks = QUERY_LAUNCH_RAYS / 256u;  // (the stack strip is the queries')
    if (blocks > waves) blocks = waves;
    return (uint32_t)blocks;
}

// radiance_kernel on a grid of at most cu_count * RADIANCE_BLOCKS_PER_CU workgroups, then radiance_resolve_kernel.
hipError_t launch_radiance(bool compact, const SceneDev& sc, const RadianceDev& rd, int cu_count, hipStream_t stream);

}  // namespace rayrs
