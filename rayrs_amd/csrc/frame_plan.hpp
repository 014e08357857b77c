// frame_plan.hpp -- what a frame is, as plain numbers worked out before anything is allocated or enqueued: its route and
// walk, its items and segments, the path pool, the grids, and the bytes of every buffer a render reserves.  frame_plan.cpp
// calls nothing in HIP and needs no scene handle (tests/frame_plan_probe.cpp links it alone); render.cpp fills the
// kernels' arguments from these numbers and the scene's buffers.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/rayrs_hip.h"
#include "layout.h"
#include "rayrs_lab.h"
#include "wavefront.h"

namespace rayrs {

constexpr uint32_t LOCAL_SEGMENT_ITEMS = 1u << 27;  // items per launch of the local-pool kernel
constexpr uint32_t LOCAL_MAX_SEGMENTS = 64;
constexpr size_t POOL_SLOT_BYTES = sizeof(PathSlot) + 4 * sizeof(double) + 1u;  // a slot record, its light entry, its state byte

// a pool of at least `slots` slots in whole windows (WfDev::np: a multiple of 1024)
inline uint64_t pool_whole_windows(uint64_t slots) { return (slots + 1023ull) & ~1023ull; }

// The route and the walk of a frame.  exact: the default walk, asked for or by the camera rule of
// rayrs_render_params.fast_traversal; the local-pool route's walk is exact whatever it says.
struct FrameWalk {
    bool use_local, exact;
};
inline FrameWalk frame_route(bool local_ok, const rayrs_tuning& tuning, uint32_t fast_traversal, bool camera_far) {
    return FrameWalk{local_ok && tuning.local_pool != 1u, fast_traversal == 0u || camera_far};
}
// which of a scene's three trees a frame walks: the fast walk [0] (or [1] with rayrs_lab_tuning.gate_tree), the default walk [2]
// if the scene has a hot group and the lab has not switched it off, else [1]
inline int walk_index(bool exact, bool has_hot, const rayrs_lab_tuning& lab) {
    if (!exact) return lab.gate_tree ? 1 : 0;
    return (has_hot && lab.hot_group != 0xffffffffu) ? 2 : 1;
}
bool camera_is_far(const double root_box[6], double small_extent, const double origin[3]);

// what the plan needs of one walk: the traversal kernel's workgroups per CU (the occupancy query's answer), the entries of
// a lane's stack (at least 1) and how many of them live in LDS
struct WalkNumbers {
    uint32_t blocks_per_cu, stack_depth, stack_lds;
};
// words of the traversal stacks' overflow strip for a launch of `threads` threads: the entries beyond the LDS part
inline size_t stack_spill_words(uint32_t stack_depth, uint32_t stack_lds, uint64_t threads) { return (size_t)(stack_depth - stack_lds) * threads; }
inline size_t stack_spill_words(const SceneDev& sc, uint64_t threads) { return stack_spill_words(sc.stack_depth, sc.stack_lds, threads); }

// The traversal kernel's launch settings on a pool of np slots, for a render and for rayrs_test_trace alike: its grid, its
// scheduling thresholds (rayrs_lab.h) and the windows dealt round robin.
struct TravPlan {
    uint32_t blocks, refill_min, leaf_min, leaf_wait, static_windows;
    void fill(RenderDev& rp) const { rp.refill_min = refill_min, rp.leaf_min = leaf_min, rp.leaf_wait = leaf_wait, rp.static_windows = static_windows; }
};
TravPlan plan_traversal(const rayrs_lab_tuning& lab, bool exact, uint32_t cu_count, uint32_t blocks_per_cu, uint32_t np, uint32_t window_slots);

struct FrameInputs {
    uint32_t x_pixels, y_pixels;  // the camera's
    rayrs_render_params params;
    uint32_t sample0;
    bool has_list;                // a film pass over a tile list of n_list tiles
    uint32_t n_list;
    uint32_t cu_count;
    bool local_ok;                // the scene fits the local-pool route ...
    uint32_t local_blocks_per_cu; // ... with this many of its workgroups per CU
    bool has_hot;                 // the scene has a hot group (walk [2])
    WalkNumbers walk[3];          // by walk_index
    rayrs_tuning tuning;
    rayrs_lab_tuning lab;
    bool any_emitter;             // a surface emits
    uint32_t window_slots;        // wf_window_slots()
    bool camera_far;              // camera_is_far
};

struct FramePlan {
    bool use_local, exact;  // use_local: the local-pool route (else the streaming route)
    int walk;               // walk_index(exact)
    bool hot_group;         // the streaming route on the hot-group tree
    // the frame's items: the (pixel, chunk) pairs of this rank's 8x8 tiles -- or, for a film pass over a tile list, of the list's
    uint32_t chunk, nchunks;
    TileShare share;        // (n_local_tiles: at most the list's)
    uint64_t total_items;
    uint64_t partial_need;     // item sums the frame needs at a time
    // the local-pool route: launches over segments of seg_tiles whole tiles, by local_blocks workgroups
    uint64_t tile_items, seg_tiles, seg_items;
    uint32_t local_blocks;  // (0: not this route)
    // the streaming route: live_total slots in a pool of np, the traversal grid, the gen / hit / miss kernels' common grid
    uint64_t live_total;
    uint32_t np, flat_blocks;  // (np 0, and with it flat_blocks and spill_words: not this route)
    TravPlan trav;
    size_t spill_words;
    bool eager_light;
    // what render_enqueue reserves
    size_t partial_bytes, local_light_bytes, pool_bytes, wave_items_bytes, spill_bytes;
};

// RAYRS_OK, or RAYRS_UNSUPPORTED for a frame of 2^32 items and more (p then holds the items and nothing behind them)
int plan_frame(const FrameInputs& in, FramePlan& p);

}  // namespace rayrs
