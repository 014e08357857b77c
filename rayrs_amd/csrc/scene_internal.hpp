// scene_internal.hpp -- the handles behind include/rayrs_hip.h, shared by the host units (abi.cpp, scene_device.cpp, render.cpp, film_abi.cpp, selftest.cpp, multi_device.cpp ...).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/rayrs_hip.h"
#include "device_mem.hpp"
#include "film.h"
#include "frame_plan.hpp"
#include "local_pool.h"
#include "rayrs_lab.h"
#include "scene_host.hpp"
#include "wavefront.h"

struct rayrs_objects {
    rayrs::ObjectList list;
};

// The work counters that layout.h Counters and rayrs_render_stats share under one name each, in Counters' order
// (surface_hits[8], which sits among them, apart): X(name) once per counter.
#define RAYRS_WORK_COUNTERS(X)                                                                                  \
    X(rays) X(paths) X(nan_pixels) X(neg_pixels)                                                                \
    X(interior_visits) X(tri_tests) X(sphere_tests) X(plane_tests) X(escaped_paths)                             \
    X(step_wave) X(step_lane) X(inner_wave) X(leaf_wave)                                                        \
    X(interior_ticks) X(leaf_ticks) X(refill_ticks)                                                             \
    X(direct_rays) X(pre_rays) X(pre_root_records) X(hot_lane) X(hot_prim_tests) X(hot_tri_divided)
#ifndef RAYRS_LAB_TICKS
#define RAYRS_COUNT_ONE(name) +1
static_assert(((RAYRS_WORK_COUNTERS(RAYRS_COUNT_ONE)) + 8) * sizeof(unsigned long long) == sizeof(rayrs::Counters),
              "RAYRS_WORK_COUNTERS and surface_hits[8] are all of Counters");
#undef RAYRS_COUNT_ONE
#endif

struct rayrs_scene {
    rayrs::FlatScene flat;
    std::vector<rayrs::SurfaceDev> surfaces;
    uint64_t n_objects = 0;
    int device = -1;
    // Every device resource below has an owner (device_mem.hpp): the destructor waits for a render in flight on the
    // scene's device, then the members release themselves.
    ~rayrs_scene();
    rayrs::DevBuf d_prims, d_surfaces, d_hdri;
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
    uint32_t stack_depth(int which) const { return tree(which).stack_need ? tree(which).stack_need : 1; }  // entries of a lane's stack
    rayrs::DevBuf d_hot;  // one HotGroupDev
    int walk_index(bool exact) const { return rayrs::walk_index(exact, flat.has_hot, lab); }  // which of the three a frame walks
    uint64_t device_bytes = 0;
    // The path pool of the streaming route (render.cpp enqueue_streaming): slots, state bytes, control words,
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
    // Everything a frame in flight uses, and what is kept of it between frames: one frame per scene at a time.
    struct Frame {
        rayrs::DevBuf d_counters;
        rayrs::DevBuf d_partial;    // the item sums: 3 doubles per (pixel, chunk) item, grown to the largest frame so far
        rayrs::DevBuf d_next_item;  // the device-wide item counter
        rayrs::Event ev[3];         // a frame's start, the end of its path rounds, the end of its resolve
        hipStream_t last_stream = nullptr;
        bool pending = false;
        uint32_t rounds = 0;
        Pool pool;
        rayrs::DevBuf d_local_light;      // 4 doubles per resident path
        rayrs::DevBuf d_local_items;      // one item counter per launch segment
        // What the frame took, written when it is enqueued: all that rayrs_render_finish reports of route and walk.
        struct Taken {
            bool use_local;  // the local-pool route
            bool exact;      // the exact walk (asked for, or a far camera: frame_plan.cpp camera_is_far)
            bool hot_group;  // the streaming route's default walk on the hot-group tree
        } taken = {};
        // The one wait for a frame in flight (the scene's device is current).  Touches no error text.
        hipError_t wait();
    };
    Frame frame;
    // What the ray queries (query_abi.cpp) keep between calls; nothing of it is a render's.
    struct Queries {
        rayrs::DevBuf d_prim_object;   // flat.prim_object, uploaded by the first closest-hit query (scene_device.cpp)
        bool has_prim_object = false;
        rayrs::DevBuf d_stack_spill;   // the traversal stacks' overflow of one launch, reserved at its largest size
        rayrs::Event ev_done;          // behind the last launch that used the strip: the next query's stream waits for it
        bool has_event = false, strip_in_use = false;
        rayrs::DevBuf d_origin, d_direction, d_t_max, d_t, d_object, d_normal, d_occluded;  // the host forms' staging
    };
    Queries queries;
    // What ambient occlusion (ao_abi.cpp) keeps between calls: the host forms' staging, which is also where the image form's
    // first pass leaves its points; the traversal stacks' overflow is the queries' strip.
    struct Ao {
        rayrs::DevBuf d_position, d_normal, d_active, d_count, d_visibility;
        rayrs::DevBuf d_turns;       // the lab's two turn counters (rayrs_lab_ao_turns)
        uint32_t refill_below = 0;   // rayrs_lab_ao_refill; 0 = the default (ao_kernels.h AO_REFILL_BELOW)
    };
    Ao ao;
    // What the radiance queries (radiance_abi.cpp) keep between calls: a launch's scratch (radiance_kernels.h
    // RADIANCE_SCRATCH_BYTES: the item cursor, the items' sums and query counts), ordered between streams with the queries'
    // strip and by its event; the host forms' staging; the lab's knobs.
    struct Radiance {
        rayrs::DevBuf d_scratch;
        rayrs::DevBuf d_a, d_b, d_radiance, d_queries;
        rayrs::DevBuf d_turns;       // the lab's three turn counters (rayrs_lab_radiance_turns)
        uint32_t refill_below = 0, shade_at = 0, leaf_min = 0;  // rayrs_lab_radiance_tuning; 0 = the default (radiance_kernels.h)
    };
    Radiance radiance;
    // What the lit radiance queries (radiance_lit_abi.cpp) keep beside the radiance queries' scratch and staging, which they
    // share: the inverse of flat.prim_object (object in insertion order -> depth-first slot), made by the first call with lights.
    struct Lit {
        std::vector<uint32_t> object_prim;
    };
    Lit lit;
    // What the sky queries (radiance_sky_abi.cpp, include/rayrs_hip.h SKY SAMPLING) keep: the table of the host scene's HDRI
    // (radiance_sky_table.h: M, C, A), built by the first sky call of any kind -- a host-only scene has one --, its total T, and
    // the device copy, uploaded by the first call that launches.
    struct Sky {
        std::vector<double> table;
        double total = 0.0;
        bool built = false, uploaded = false;
        rayrs::DevBuf d_table;
    };
    Sky sky;
    // What SH probes (radiance_probe_abi.cpp, include/rayrs_hip.h SH PROBES) keep beside the radiance queries' scratch and
    // staging, which they share: the projection's chunk sums (radiance_probe_kernels.h PROBE_CHUNK_BYTES, a fixed size),
    // allocated by the scene's first probe call and used in the scratch's order.
    struct Probes {
        rayrs::DevBuf d_chunks;
    };
    Probes probes;
    // Scenes whose walk tree is at most one record are rendered by local_pool.hip: every path resident in LDS.
    bool local_ok = false;
    rayrs::LocalScene local = {};
    int local_blocks_per_cu = 1;      // local-pool kernel, from the occupancy query with the scene's LDS size
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
// sets the scene's device (>= 0) and waits for what the scene still has in flight on it (render.cpp)
int scene_settle(rayrs_scene* s);
// the bytes of a w x h frame in an out_format
inline size_t frame_bytes(uint32_t w, uint32_t h, uint32_t out_format) {
    return (size_t)w * h * 3 * (out_format == RAYRS_OUT_F64 ? 8 : 4);
}
// the gating boxes of a scene the local-pool route can render, before the upload (scene_device.cpp)
void scene_configure_local(rayrs_scene* s);
// uploads s->flat to s->device and sizes the traversal kernel's LDS (scene_device.cpp)
int scene_upload(rayrs_scene* s);
// sizes the traversal workgroup's LDS again, after the lab knobs changed (scene_device.cpp)
int scene_configure_traversal(rayrs_scene* s);
// what a render hands its kernels, for the self tests too (scene_device.cpp)
SceneDev make_scene_dev(const rayrs_scene* s, bool exact);
CameraDev make_camera_dev(const rayrs_camera* c);
// the device copy of flat.prim_object (depth-first slot -> object in insertion order), uploaded at the first call
// (scene_device.cpp; the scene's device is current)
int scene_prim_object(rayrs_scene* s, const uint32_t** out);
// the route and the walk of a frame with these settings (frame_plan.hpp frame_route, camera_is_far)
FrameWalk frame_walk(const rayrs_scene* s, const rayrs_camera* c, uint32_t fast_traversal);
// the traversal kernel's settings on a pool of np slots of this scene (frame_plan.hpp plan_traversal)
TravPlan trav_settings(const rayrs_scene* s, bool exact, uint32_t np);
WfDev pool_wf(const DevBuf& block, uint32_t np, const DevBuf& ctl, uint32_t trav_blocks, const DevBuf& spill);
// enqueues a frame (film == nullptr, sample0 = 0: rayrs_render_launch) or a film's pass over the samples sample0 ..
// sample0 + params->spp - 1 (film_abi.cpp); render_finish waits for either and reads its counters and times (render.cpp)
int render_enqueue(rayrs_scene* scene, const rayrs_camera* camera, const rayrs_render_params* params, uint32_t sample0,
                   const FilmPassDev* film, void* out_device, void* hip_stream);
int render_finish(rayrs_scene* scene, rayrs_render_stats* stats);
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
