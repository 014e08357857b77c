// scene_internal.hpp -- the handles behind include/rayrs_hip.h, shared by abi.cpp, selftest.cpp and multi_device.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/rayrs_hip.h"
#include "device_mem.hpp"
#include "film.h"
#include "local_pool.h"
#include "rayrs_lab.h"
#include "scene_host.hpp"
#include "wavefront.h"

struct rayrs_objects {
    rayrs::ObjectList list;
};

struct rayrs_scene {
    rayrs::FlatScene flat;
    std::vector<rayrs::SurfaceDev> surfaces;
    uint64_t n_objects = 0;
    int device = -1;
    // Every device resource below has an owner (device_mem.hpp): the destructor waits for a render in flight on the
    // scene's device, then the members release themselves.
    ~rayrs_scene();
    rayrs::DevBuf d_prims, d_surfaces, d_hdri, d_counters;
    rayrs::DevBuf d_partial;  // the item sums: 3 doubles per (pixel, chunk) item, grown to the largest frame so far
    rayrs::Event ev[3];       // a frame's start, the end of its path rounds, the end of its resolve
    hipStream_t last_stream = nullptr;
    bool pending = false;
    int cu_count = 0;
    // How the traversal kernel walks each of the scene's two trees: [0] FlatScene::walk (rayrs_render_params.fast_traversal),
    // [1] FlatScene::gate (the default walk).
    struct Walk {
        rayrs::DevBuf d_nodes;
        int blocks_per_cu = 0;       // traversal kernel, from the occupancy query
        uint32_t stack_lds = 1;      // traversal stack entries kept in LDS
        uint32_t hot_records = 0;    // leading records kept in LDS
        uint32_t leafq = 0;          // leaf groups a lane of the default walk may have waiting in LDS (0: the fast walk's tree)
    };
    // [2] FlatScene::gate_hot (the default walk on a scene with a hot group: layout.h HotGroupDev).
    Walk trav[3];
    const rayrs::WalkTree& tree(int which) const { return which == 2 ? flat.gate_hot : which == 1 ? flat.gate : flat.walk; }
    rayrs::DevBuf d_hot;  // one HotGroupDev
    // which of the three a frame walks: the fast walk [0] (or [1] with rayrs_lab_tuning.gate_tree), the default walk [2] if the
    // scene has a hot group and the lab has not switched it off, else [1]
    int walk_index(bool exact) const {
        if (!exact) return lab.gate_tree ? 1 : 0;
        return (flat.has_hot && lab.hot_group != 0xffffffffu) ? 2 : 1;
    }
    uint64_t device_bytes = 0;
    // The path pool of the streaming route (abi.cpp rayrs_render_launch): slots, state bytes, control words,
    // per-wave item ranges and traversal-stack overflow strips, kept between renders.
    struct Pool {
        rayrs::DevBuf block;          // one allocation holding the slot records, the light entries and the state bytes
        rayrs::DevBuf d_ctl;          // one WfCtl
        rayrs::DevBuf d_wave_items;   // two counters per wave of the gen / hit / miss grid
        rayrs::DevBuf d_stack_spill;  // one word per traversal thread and stack entry beyond the LDS part
        rayrs::PinnedBuf h_live;      // two words: live_slots read-backs
        rayrs::Event ev_batch[2];
        std::vector<rayrs::Event> ev_round;  // four per round: around the traversal, hit and miss launches
        uint32_t timed_rounds = 0;
    };
    Pool pool;
    rayrs::DevBuf d_next_item;  // the device-wide item counter
    uint32_t rounds = 0;
    // Scenes whose walk tree is at most one record are rendered by local_pool.hip: every path resident in LDS.
    bool local_ok = false;
    bool last_local = false;          // the render in flight took that route
    bool last_exact = false;          // ... with the exact walk (asked for, or a far camera: abi.cpp camera_is_far)
    rayrs::LocalScene local = {};
    int local_blocks_per_cu = 1;      // local-pool kernel, from the occupancy query with the scene's LDS size
    rayrs::DevBuf d_local_light;      // 4 doubles per resident path
    rayrs::DevBuf d_local_items;      // one item counter per launch segment
    // rayrs_render_multi: this rank's stream and zeroed full-size framebuffer, kept between calls
    rayrs::Stream multi_stream;
    rayrs::DevBuf multi_out;
    rayrs_tuning tuning = {};  // zeros = defaults (rayrs_scene_set_tuning)
    rayrs_lab_tuning lab = {};  // development knobs (rayrs_lab.h), zeros = defaults
};

namespace rayrs {
// thread-local text behind rayrs_last_error()
void set_last_error(const std::string& text);
int hip_fail(hipError_t e, const char* what);
// sets the scene's device (>= 0) and waits for what the scene still has in flight on it (abi.cpp)
int scene_settle(rayrs_scene* s);
// the bytes of a w x h frame in an out_format
inline size_t frame_bytes(uint32_t w, uint32_t h, uint32_t out_format) {
    return (size_t)w * h * 3 * (out_format == RAYRS_OUT_F64 ? 8 : 4);
}
// uploads s->flat to s->device and sizes the traversal kernel's LDS (abi.cpp)
int scene_upload(rayrs_scene* s);
// what a render hands its kernels, for the self tests too (abi.cpp)
SceneDev make_scene_dev(const rayrs_scene* s, bool exact);
CameraDev make_camera_dev(const rayrs_camera* c);
// The route and the walk of a frame with these settings (abi.cpp).  exact: the default walk, asked for or by the camera rule of
// rayrs_render_params.fast_traversal; the local-pool route's walk is exact whatever it says.
struct FrameWalk {
    bool use_local, exact;
};
FrameWalk frame_walk(const rayrs_scene* s, const rayrs_camera* c, uint32_t fast_traversal);
// words of the traversal stacks' overflow strip for a launch of `threads` threads: the entries beyond the LDS part
inline size_t stack_spill_words(const SceneDev& sc, uint64_t threads) { return (size_t)(sc.stack_depth - sc.stack_lds) * threads; }
uint32_t trav_settings(const rayrs_scene* s, bool exact, uint32_t np, RenderDev& rp);
constexpr size_t POOL_SLOT_BYTES = sizeof(PathSlot) + 4 * sizeof(double) + 1u;  // a slot record, its light entry, its state byte
WfDev pool_wf(const DevBuf& block, uint32_t np, const DevBuf& ctl, uint32_t trav_blocks, const DevBuf& spill);
// enqueues a frame (film == nullptr, sample0 = 0: rayrs_render_launch) or a film's pass over the samples sample0 ..
// sample0 + params->spp - 1 (film_abi.cpp); rayrs_render_finish waits for either (abi.cpp)
int render_enqueue(rayrs_scene* scene, const rayrs_camera* camera, const rayrs_render_params* params, uint32_t sample0,
                   const FilmPassDev* film, void* out_device, void* hip_stream);
}  // namespace rayrs

#define HIP_TRY(expr)                                       \
    do {                                                    \
        hipError_t _e = (expr);                             \
        if (_e != hipSuccess) return rayrs::hip_fail(_e, #expr); \
    } while (0)

#define RAYRS_TRY(expr)                \
    do {                               \
        const int _s = (expr);         \
        if (_s != RAYRS_OK) return _s; \
    } while (0)

// No exception may cross the C boundary (a std::bad_alloc from a vector would otherwise end the host process).
#define RAYRS_GUARDED(...)                                   \
    try {                                                    \
        __VA_ARGS__                                          \
    } catch (const std::bad_alloc&) {                        \
        rayrs::set_last_error("out of host memory");         \
        return RAYRS_OOM;                                    \
    } catch (const std::exception& e) {                      \
        rayrs::set_last_error(e.what());                     \
        return RAYRS_INVALID_ARG;                            \
    } catch (...) {                                          \
        rayrs::set_last_error("unknown exception");          \
        return RAYRS_INVALID_ARG;                            \
    }
