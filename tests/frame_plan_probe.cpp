// Stand-alone host program of tests/test_frame_plan.py: plans one frame per line of standard input with
// rayrs_amd/csrc/frame_plan.cpp (linked alone: no HIP runtime, no scene handle) and prints the plan's numbers, one line per
// frame.  A line is "key=value" words; what it leaves out is 0.  bpc / depth / lds set all three walks, bpcN / depthN / ldsN
// walk N; the lab.* keys are rayrs_lab_tuning's fields.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "../rayrs_amd/csrc/frame_plan.hpp"

using namespace rayrs;

static bool set_field(FrameInputs& in, const std::string& k, uint64_t v) {
    const uint32_t u = (uint32_t)v;
#define FIELD(name, target) \
    if (k == name) return (target) = u, true;
    FIELD("w", in.x_pixels) FIELD("h", in.y_pixels) FIELD("spp", in.params.spp) FIELD("chunk", in.params.sample_chunk)
    FIELD("rank", in.params.tile_rank) FIELD("ranks", in.params.tile_ranks) FIELD("fast", in.params.fast_traversal)
    FIELD("sample0", in.sample0) FIELD("has_list", in.has_list) FIELD("n_list", in.n_list) FIELD("cus", in.cu_count)
    FIELD("local_ok", in.local_ok) FIELD("local_bpc", in.local_blocks_per_cu) FIELD("has_hot", in.has_hot)
    FIELD("pool_slots", in.tuning.pool_slots) FIELD("no_local", in.tuning.local_pool) FIELD("emitter", in.any_emitter)
    FIELD("window", in.window_slots) FIELD("far", in.camera_far)
    FIELD("lab.refill_min", in.lab.refill_min) FIELD("lab.leaf_min", in.lab.leaf_min) FIELD("lab.static_pct", in.lab.static_pct)
    FIELD("lab.trav_blocks_per_cu", in.lab.trav_blocks_per_cu) FIELD("lab.eager_light", in.lab.eager_light)
    FIELD("lab.local_segment_items", in.lab.local_segment_items) FIELD("lab.gate_tree", in.lab.gate_tree)
    FIELD("lab.hot_group", in.lab.hot_group) FIELD("lab.leaf_wait", in.lab.leaf_wait)
    FIELD("lab.flat_blocks_per_cu", in.lab.flat_blocks_per_cu)
#undef FIELD
    bool known = false;
    for (int x = 0; x < 3; x++) {
        const std::string n = std::to_string(x);
        if (k == "bpc" || k == "bpc" + n) in.walk[x].blocks_per_cu = u, known = true;
        if (k == "depth" || k == "depth" + n) in.walk[x].stack_depth = u, known = true;
        if (k == "lds" || k == "lds" + n) in.walk[x].stack_lds = u, known = true;
    }
    return known;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        FrameInputs in;
        std::memset(&in, 0, sizeof(in));
        std::istringstream words(line);
        std::string word;
        while (words >> word) {
            const size_t eq = word.find('=');
            if (eq == std::string::npos || !set_field(in, word.substr(0, eq), std::strtoull(word.c_str() + eq + 1, nullptr, 0))) {
                std::fprintf(stderr, "frame_plan_probe: bad word '%s'\n", word.c_str());
                return 2;
            }
        }
        FramePlan p;
        const int status = plan_frame(in, p);
        std::printf("status=%d use_local=%d exact=%d walk=%d hot_group=%d chunk=%u nchunks=%u tiles_x=%u tiles_y=%u n_local_tiles=%u "
                    "total_items=%" PRIu64 " partial_need=%" PRIu64 " tile_items=%" PRIu64 " seg_tiles=%" PRIu64 " seg_items=%" PRIu64
                    " local_blocks=%u live_total=%" PRIu64 " np=%u flat_blocks=%u trav_blocks=%u refill_min=%u leaf_min=%u leaf_wait=%u "
                    "static_windows=%u spill_words=%zu eager_light=%d partial_bytes=%zu local_light_bytes=%zu pool_bytes=%zu "
                    "wave_items_bytes=%zu spill_bytes=%zu\n",
                    status, (int)p.use_local, (int)p.exact, p.walk, (int)p.hot_group, p.chunk, p.nchunks, p.share.tiles_x, p.share.tiles_y,
                    p.share.n_local_tiles, p.total_items, p.partial_need, p.tile_items, p.seg_tiles, p.seg_items, p.local_blocks, p.live_total,
                    p.np, p.flat_blocks, p.trav.blocks, p.trav.refill_min, p.trav.leaf_min, p.trav.leaf_wait, p.trav.static_windows,
                    p.spill_words, (int)p.eager_light, p.partial_bytes, p.local_light_bytes, p.pool_bytes, p.wave_items_bytes, p.spill_bytes);
    }
    return 0;
}
