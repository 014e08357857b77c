// frame_plan.cpp -- a frame's plan (frame_plan.hpp): arithmetic only.  Nothing here calls the HIP runtime or sees a scene
// handle, so the unit links into a host program on its own (tests/frame_plan_probe.cpp).
#include "frame_plan.hpp"

#include "local_pool.h"

namespace rayrs {

namespace {
constexpr uint32_t FLAT_BLOCKS_PER_CU_MIN = 8, FLAT_BLOCKS_PER_CU_MAX = 24;  // the gen / hit / miss kernels' common grid (rayrs_lab_tuning.flat_blocks_per_cu)
}  // namespace

// The fast walk's leaf boxes are a bet on the reference's arithmetic that was measured to hold for rays from nearby and
// to fail, a few times in 10^4, for rays aimed along a primitive's plane from far away (include/rayrs_hip.h
// fast_traversal; profiles/r04_tight_leaves.txt).  What decides is the distance in PRIMITIVE sizes (the error of the
// computed hit point is about eps * distance / angle against a widening of 1/64 of the primitive): failures were seen from
// 6,000 primitive sizes up, none within 4,000 (sheets of 6 ... 400 quads per side: scripts/fuzz_traversal.py).
// A frame whose camera is farther from the root Node's box than RAYRS_FAR_DIAGONALS times that box's diagonal, or than
// RAYRS_FAR_PRIMITIVES times the scene's small primitives (the 5th percentile of their largest extents), takes the
// default walk whatever was asked (rayrs_render_stats.exact_walk says which walk a frame took).  This guards PRIMARY
// rays only: a bounced ray from a large surface to a finely tessellated one (the headline scene's floor to its mesh)
// is thousands of small-primitive sizes long and makes the bet all the same -- the fast walk stays a bet.
constexpr double RAYRS_FAR_DIAGONALS = 8.0;
constexpr double RAYRS_FAR_PRIMITIVES = 4096.0;
bool camera_is_far(const double root_box[6], double small_extent, const double origin[3]) {
    const double* b = root_box;
    double d2 = 0.0, e2 = 0.0;
    for (int a = 0; a < 3; a++) {
        const double lo = b[2 * a], hi = b[2 * a + 1], o = origin[a];
        const double out = o < lo ? lo - o : (o > hi ? o - hi : 0.0);
        d2 += out * out;
        e2 += (hi - lo) * (hi - lo);
    }
    // (a box or an origin that is not a number compares false: the walk that was asked for, as for any other frame)
    const double small = small_extent;
    return d2 > RAYRS_FAR_DIAGONALS * RAYRS_FAR_DIAGONALS * e2 || (small > 0.0 && d2 > RAYRS_FAR_PRIMITIVES * RAYRS_FAR_PRIMITIVES * small * small);
}

TravPlan plan_traversal(const rayrs_lab_tuning& lab, bool exact, uint32_t cu_count, uint32_t blocks_per_cu, uint32_t np, uint32_t window_slots) {
    TravPlan t;
    t.refill_min = lab.refill_min ? lab.refill_min : 52u;
    // (a leaf phase once this many lanes stand on a leaf: 24 where a leaf is one primitive -- the fast walk's tree: 612 -> 604 ms
    // of traversal on the headline frame against 32 --, 32 where it is a group of up to four -- the default walk: 988 -> 962 ms
    // against 24)
    t.leaf_min = lab.leaf_min ? lab.leaf_min : (exact ? 48u : lab.gate_tree ? 32u : 24u);
    // (the default walk: its lanes walk on while their leaf groups wait, so a leaf phase may wait for more of them -- or for
    // leaf_wait lanes that can do nothing else; scripts/sim/walk_sched_sim.py, swept on the GPU: profiles/r06_leaf_queue.txt)
    t.leaf_wait = lab.leaf_wait ? lab.leaf_wait : 16u;
    // (pre-tested rays -- a scene with a hot group, wavefront.hip finish_rays -- wanted a refill_min of 56 while a lane stood idle
    // on its leaf: 664 -> 659 ms of traversal, profiles/r06_tuning_sweep.txt; with the leaf groups set aside 52 is best again:
    // 626 -> 619 ms, profiles/r06_leaf_queue.txt)
    uint32_t trav_bpc = blocks_per_cu;
    if (lab.trav_blocks_per_cu && lab.trav_blocks_per_cu < trav_bpc) trav_bpc = lab.trav_blocks_per_cu;
    t.blocks = cu_count * trav_bpc;
    // whole round-robin rounds covering about static_pct % of the pool's windows
    const uint32_t static_pct = lab.static_pct ? lab.static_pct : 50u;  // (rayrs_lab_set: at most 100)
    const uint64_t n_waves = (uint64_t)t.blocks * 4u;
    t.static_windows = (uint32_t)((uint64_t)(np / window_slots) * static_pct / 100u / n_waves * n_waves);
    return t;
}

int plan_frame(const FrameInputs& in, FramePlan& p) {
    const rayrs_lab_tuning& lab = in.lab;
    const rayrs_render_params& params = in.params;
    p = FramePlan{};
    p.chunk = (params.sample_chunk == 0 || params.sample_chunk >= params.spp) ? params.spp : params.sample_chunk;
    p.nchunks = (params.spp + p.chunk - 1) / p.chunk;
    p.share = tile_share(in.x_pixels, in.y_pixels, params.tile_rank, params.tile_ranks);
    if (in.has_list && in.n_list < p.share.n_local_tiles) p.share.n_local_tiles = in.n_list;  // (at most the share's tiles)
    p.total_items = (uint64_t)p.share.n_local_tiles * p.nchunks * 64ull;
    if (p.total_items >= (1ull << 32)) return RAYRS_UNSUPPORTED;
    // Item sums: 24 bytes per (pixel, chunk) item, added per pixel in chunk order by the resolve kernel.  The streaming
    // kernels finish items in no particular order, so the array covers the frame.  The local-pool route renders the frame
    // as a sequence of launches over segments of whole tiles and resolves each segment behind its launch: one segment's
    // worth is all it needs (config 4: 3.2 GB instead of 25.8).
    const FrameWalk walk = frame_route(in.local_ok, in.tuning, params.fast_traversal, in.camera_far);
    p.use_local = walk.use_local, p.exact = walk.exact;
    p.walk = walk_index(p.exact, in.has_hot, lab);
    p.hot_group = !p.use_local && p.exact && p.walk == 2;
    p.tile_items = (uint64_t)p.nchunks * 64u;
    uint64_t seg_want = lab.local_segment_items ? lab.local_segment_items : LOCAL_SEGMENT_ITEMS;
    // (a frame stays within LOCAL_MAX_SEGMENTS launches: larger segments rather than a refused frame)
    if ((p.total_items + seg_want - 1) / seg_want > LOCAL_MAX_SEGMENTS) seg_want = (p.total_items + LOCAL_MAX_SEGMENTS - 1) / LOCAL_MAX_SEGMENTS;
    p.seg_tiles = (seg_want + p.tile_items - 1) / p.tile_items > 0 ? (seg_want + p.tile_items - 1) / p.tile_items : 1;
    p.seg_items = p.seg_tiles * p.tile_items;
    p.partial_need = p.use_local && p.seg_items < p.total_items ? p.seg_items : p.total_items;
    if (p.use_local && p.seg_items >= (1ull << 32)) return RAYRS_UNSUPPORTED;  // (one tile's chunks alone: spp beyond 2^27)
    // LP_WPS workgroups of four waves per CU; fewer when the frame has fewer items than resident paths
    p.local_blocks = in.cu_count * in.local_blocks_per_cu;
    const uint64_t most_items = p.total_items < p.seg_items ? p.total_items : p.seg_items;
    const uint64_t want_blocks = (most_items + 4u * LP_PATHS_PER_WAVE - 1) / (4u * LP_PATHS_PER_WAVE);
    if (want_blocks < p.local_blocks) p.local_blocks = (uint32_t)(want_blocks ? want_blocks : 1);
    if (!p.use_local || p.total_items == 0) p.local_blocks = 0;

    // ---- path pool.  A traversal launch works through the whole pool, and its ramp-up
    // and drain are a fixed cost, so large pools win even when that leaves only one or two
    // items per slot -- up to the point where the hit and miss kernels lose more to the larger
    // footprint.  Swept on the headline frame with one-line slots: 24 M slots 1520 ms, 32 M 1516,
    // 48 M 1497, 64 M 1467, 96 M 1468, 128 M 1481, 192 M 1498 (round 1, 192-byte slots: 32 M).
    // Swept again on round 3's kernels (the traversal kernel faster, its fixed cost per launch the same): 64 M 1369 ms,
    // 80 M 1372, 96 M 1368, 112 M 1353, 128 M 1356, 160 M 1353, 192 M 1350: 112 M slots (18 GB of the 288 GB), 84 rounds.
    // And on round 6's (the hit kernel at three waves per SIMD, the cheap queries answered by the kernels that make the rays):
    // 80 M 1298 ms, 96 M 1290, 112 M 1276, 128 M 1278, 144 M 1267, 160 M 1250, 192 M 1250, 224 M 1246, 256 M 1242, 320 M 1242
    // (profiles/r06_leaf_queue.txt (12)): 256 M slots (43 GB), 52 rounds.
    // A frame should also last some tens of rounds, or filling and draining the pool is all it does: at most one
    // slot per 12 samples -- which is what a one-eighth tile share of the headline frame gets (44.7 M: 33.5 M 189 ms,
    // 48 M 184, 64 M 186).
    constexpr uint64_t POOL_MAX_SLOTS = 1ull << 28;
    uint64_t np64 = p.total_items;
    if (np64 > POOL_MAX_SLOTS) np64 = POOL_MAX_SLOTS;
    {
        const uint64_t samples = p.share.n_local_tiles * 64ull * params.spp;
        const uint64_t by_work = samples / 12u > (1ull << 20) ? samples / 12u : (1ull << 20);
        if (np64 > by_work) np64 = by_work;
    }
    if (in.tuning.pool_slots) np64 = in.tuning.pool_slots;
    if (np64 > p.total_items) np64 = p.total_items;
    p.live_total = np64;
    const bool streaming = !p.use_local && p.total_items > 0;  // (the local-pool route keeps its paths in LDS)
    p.np = streaming ? (uint32_t)pool_whole_windows(p.live_total) : 0u;
    const WalkNumbers& w = in.walk[p.walk];
    p.trav = plan_traversal(lab, p.exact, in.cu_count, w.blocks_per_cu, p.np, in.window_slots);
    p.spill_words = streaming ? stack_spill_words(w.stack_depth, w.stack_lds, (uint64_t)p.trav.blocks * 256u) : 0;

    // A path's light lives in a side array and only while it is not +0 (wavefront.h PathSlot).  Where a surface
    // emits, paths do get light, and the hit and miss kernels request the side array's entry together with the
    // slot instead of after it.
    p.eager_light = lab.eager_light != 0u || in.any_emitter;

    // the gen, hit and miss kernels run with this one grid, so wave w means the same windows in all three: one
    // wave per window, at most 8 ... 24 workgroups per CU (below)
    const uint32_t n_windows = p.np / in.window_slots;
    p.flat_blocks = (n_windows + 3u) / 4u;
    // (8 ... 24 workgroups per CU, so that a wave has about nine windows: with the hit kernel at three resident workgroups
    // per CU a finer grid evens out the end of a launch -- hit 411 -> 404 ms on the headline's 218 k windows at 24 -- but
    // a wave that gets three windows spends its time on its first and last batch: config 3's 87 k windows want 8 or 9
    // (198 against 200.5 ms at 24); profiles/r06_leaf_queue.txt (9))
    uint32_t per_cu = lab.flat_blocks_per_cu;
    if (!per_cu) {
        per_cu = n_windows / (36u * in.cu_count);
        per_cu = per_cu < FLAT_BLOCKS_PER_CU_MIN ? FLAT_BLOCKS_PER_CU_MIN : per_cu > FLAT_BLOCKS_PER_CU_MAX ? FLAT_BLOCKS_PER_CU_MAX : per_cu;
    }
    const uint32_t flat_cap = in.cu_count * per_cu;
    if (p.flat_blocks > flat_cap) p.flat_blocks = flat_cap;

    p.partial_bytes = (size_t)p.partial_need * 3 * sizeof(double);
    p.local_light_bytes = (size_t)p.local_blocks * 4u * LP_PATHS_PER_WAVE * 4 * sizeof(double);
    p.pool_bytes = (size_t)p.np * POOL_SLOT_BYTES;
    p.wave_items_bytes = (size_t)p.flat_blocks * 4u * 2 * sizeof(unsigned long long);
    p.spill_bytes = p.spill_words * sizeof(uint32_t);
    return RAYRS_OK;
}

}  // namespace rayrs
