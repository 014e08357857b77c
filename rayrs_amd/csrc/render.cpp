// render.cpp -- a render as plan (frame_plan.cpp: arithmetic only), reserve, enqueue, and its end: the wait, the counters and
// the HIP-event times.  One frame is in flight per scene at a time (scene_internal.hpp rayrs_scene::Frame).
#include <hip/hip_runtime.h>

#include <cstring>

#include "film.h"
#include "kernels.h"
#include "local_pool.h"
#include "scene_internal.hpp"
#include "wavefront.h"

using namespace rayrs;

hipError_t rayrs_scene::Frame::wait() {
    if (!pending) return hipSuccess;
    const hipError_t e = hipStreamSynchronize(last_stream);
    if (e == hipSuccess) pending = false;
    return e;
}

int rayrs::scene_settle(rayrs_scene* scene) {
    HIP_TRY(hipSetDevice(scene->device));
    HIP_TRY(scene->frame.wait());
    return RAYRS_OK;
}

// A timed round r owns four events, pool.ev_round[4 r + k]: k = 0 before its traversal kernel, 1 behind it, 2 behind the hit
// kernel, 3 behind the miss kernel (the local-pool route: 0 and 1 around a segment's one launch).  round_event records one
// of them (and creates the round's four the first time); round_ms reads the three intervals back after the frame.
static int round_event(rayrs_scene::Pool& pl, uint32_t r, uint32_t k, hipStream_t stream) {
    while (pl.ev_round.size() < 4 * (size_t)(r + 1)) {
        Event e;
        HIP_TRY(e.create());
        pl.ev_round.push_back(std::move(e));
    }
    HIP_TRY(hipEventRecord(pl.ev_round[4 * (size_t)r + k], stream));
    return RAYRS_OK;
}

static int round_ms(const rayrs_scene* scene, uint32_t r, float ms[3]) {
    const Event* e = &scene->frame.pool.ev_round[4 * (size_t)r];
    ms[1] = ms[2] = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms[0], e[0], e[1]));
    if (scene->frame.taken.use_local) return RAYRS_OK;  // one kernel per segment
    HIP_TRY(hipEventElapsedTime(&ms[1], e[1], e[2]));
    HIP_TRY(hipEventElapsedTime(&ms[2], e[2], e[3]));
    return RAYRS_OK;
}

// rayrs_lab.h: HIP-event times of the last render's path rounds, three per round (traversal, hit, miss kernel; the
// local-pool route: its launch, 0, 0).  Returns the number of rounds; writes at most cap_rounds of them.
extern "C" int rayrs_lab_round_ms(rayrs_scene* scene, float* out, uint32_t cap_rounds) {
    if (!scene || scene->device < 0 || scene->frame.pending) return RAYRS_INVALID_ARG;
    HIP_TRY(hipSetDevice(scene->device));
    for (uint32_t r = 0; r < scene->frame.pool.timed_rounds && r < cap_rounds && out; r++) RAYRS_TRY(round_ms(scene, r, out + 3 * r));
    return (int)scene->frame.pool.timed_rounds;
}

FrameWalk rayrs::frame_walk(const rayrs_scene* s, const rayrs_camera* c, uint32_t fast_traversal) {
    return frame_route(s->local_ok, s->tuning, fast_traversal, camera_is_far(s->flat.root_box, s->flat.small_extent, c->origin));
}

CameraDev rayrs::make_camera_dev(const rayrs_camera* c) {
    CameraDev cam;
    std::memset(&cam, 0, sizeof(cam));
    for (int i = 0; i < 3; i++) {
        cam.origin[i] = c->origin[i];
        cam.e_x[i] = c->e_x[i];
        cam.e_y[i] = c->e_y[i];
        cam.z[i] = c->z[i];
    }
    cam.width = c->width;
    cam.height = c->height;
    cam.ppc = (double)c->ppc;  // `self.ppc as f64`, lib.rs:206
    cam.W = c->x_pixels;
    cam.H = c->y_pixels;
    return cam;
}

TravPlan rayrs::trav_settings(const rayrs_scene* s, bool exact, uint32_t np) {
    return plan_traversal(s->lab, exact, (uint32_t)s->cu_count, (uint32_t)s->trav[s->walk_index(exact)].blocks_per_cu, np, wf_window_slots());
}

// A pool of np slots (whole windows) in one block -- the slot records, the light entries, the state bytes -- walked by
// trav_blocks workgroups whose stacks overflow into `spill`.
WfDev rayrs::pool_wf(const DevBuf& block, uint32_t np, const DevBuf& ctl, uint32_t trav_blocks, const DevBuf& spill) {
    WfDev wf;
    std::memset(&wf, 0, sizeof(wf));
    wf.slots = block.as<PathSlot>();
    wf.light = reinterpret_cast<double*>(wf.slots + np);
    wf.state = reinterpret_cast<uint8_t*>(wf.light + (size_t)np * 4u);
    wf.ctl = ctl.as<WfCtl>();
    wf.np = np;
    wf.trav_threads = trav_blocks * 256u;
    wf.stack_spill = spill.as<uint32_t>();
    return wf;
}

// What plan_frame needs to know of the scene, the camera and the request.
static FrameInputs frame_inputs(const rayrs_scene* scene, const rayrs_camera* camera, const rayrs_render_params* params, uint32_t sample0,
                                const FilmPassDev* film) {
    FrameInputs in;
    std::memset(&in, 0, sizeof(in));
    in.x_pixels = camera->x_pixels, in.y_pixels = camera->y_pixels;
    in.params = *params;
    in.sample0 = sample0;
    in.has_list = film && film->list;
    in.n_list = in.has_list ? film->n_list : 0u;
    in.cu_count = (uint32_t)scene->cu_count;
    in.local_ok = scene->local_ok;
    in.local_blocks_per_cu = (uint32_t)scene->local_blocks_per_cu;
    in.has_hot = scene->flat.has_hot;
    for (int x = 0; x < 3; x++) in.walk[x] = WalkNumbers{(uint32_t)scene->trav[x].blocks_per_cu, scene->stack_depth(x), scene->trav[x].stack_lds};
    in.tuning = scene->tuning;
    in.lab = scene->lab;
    for (const SurfaceDev& sf : scene->surfaces)
        if (sf.emit[0] != 0.0 || sf.emit[1] != 0.0 || sf.emit[2] != 0.0) in.any_emitter = true;
    in.window_slots = wf_window_slots();
    in.camera_far = camera_is_far(scene->flat.root_box, scene->flat.small_extent, camera->origin);
    return in;
}

// The kernels' arguments of a planned frame: the plan's numbers and the scene's buffers.
struct FrameDev {
    SceneDev sc;
    CameraDev cam;
    RenderDev rp;  // complete but for `partial`
    // a film pass (rayrs_film_render): film_accumulate_kernel takes the resolve kernel's place
    bool is_film;
    FilmPassDev film;
};

static RenderDev make_render_dev(const rayrs_scene* scene, const rayrs_render_params* params, uint32_t sample0, const FramePlan& p,
                                 const FilmPassDev* film, void* out_device) {
    RenderDev rp;
    std::memset(&rp, 0, sizeof(rp));
    rp.spp = params->spp;
    rp.sample0 = sample0;
    rp.max_bounces = params->max_bounces;
    rp.seed = params->seed;
    rp.chunk = p.chunk;
    rp.nchunks = p.nchunks;
    rp.tile_rank = p.share.tile_rank, rp.tile_ranks = p.share.tile_ranks;
    rp.tiles_x = p.share.tiles_x, rp.tiles_y = p.share.tiles_y;
    rp.n_local_tiles = p.share.n_local_tiles;
    if (film && film->list) rp.tile_list = film->list;
    rp.total_items = p.total_items;
    rp.inv_nchunks = 1.0 / (double)rp.nchunks;
    rp.inv_tiles_x = 1.0 / (double)rp.tiles_x;
    rp.count_work = params->count_work ? 1u : 0u;
    rp.out_format = params->out_format;
    rp.out = out_device;
    rp.counters = scene->frame.d_counters.as<Counters>();
    rp.next_item = scene->frame.d_next_item.as<unsigned long long>();
    p.trav.fill(rp);
    return rp;
}

// ---- one launch per segment of the frame's items; a launch ends when its last path has (local_pool.hip)
static int enqueue_local(rayrs_scene* scene, const FramePlan& p, const FrameDev& d, hipStream_t stream) {
    rayrs_scene::Frame& fr = scene->frame;
    rayrs_scene::Pool& pl = fr.pool;
    const RenderDev& rp = d.rp;
    const uint64_t n_seg = (rp.total_items + p.seg_items - 1) / p.seg_items;
    for (uint64_t seg = 0; seg < n_seg; seg++) {
        LocalDev lp;
        lp.light = fr.d_local_light.as<double>();
        lp.next_item = fr.d_local_items.as<unsigned long long>() + seg;
        lp.item_base = seg * p.seg_items;
        lp.item_count = rp.total_items - lp.item_base < p.seg_items ? rp.total_items - lp.item_base : p.seg_items;
        RenderDev rseg = rp;
        rseg.partial_item0 = lp.item_base;
        const uint64_t share = lp.item_count / ((uint64_t)p.local_blocks * 4u * 16u);  // a sixteenth of a wave's share
        lp.reserve = (uint32_t)(share < 8u ? 8u : share > 256u ? 256u : share);
        if (scene->lab.local_reserve) lp.reserve = scene->lab.local_reserve;
        lp.pad = 0;
        RAYRS_TRY(round_event(pl, (uint32_t)seg, 0, stream));
        HIP_TRY(lp_launch(scene->flat.compact, rp.count_work != 0u, d.sc, scene->local, d.cam, rseg, lp, p.local_blocks, stream));
        RAYRS_TRY(round_event(pl, (uint32_t)seg, 1, stream));
        // the segment's tiles, resolved behind its launch (the next segment reuses the item-sum array)
        const uint32_t seg_lt0 = (uint32_t)(seg * p.seg_tiles), seg_n_lt = (uint32_t)(lp.item_count / p.tile_items);
        HIP_TRY(d.is_film ? launch_film_accumulate(d.cam, rseg, d.film, seg_lt0, seg_n_lt, stream) : launch_resolve(d.cam, rseg, seg_lt0, seg_n_lt, stream));
        pl.timed_rounds = (uint32_t)seg + 1;
    }
    fr.rounds = (uint32_t)n_seg;
    return RAYRS_OK;
}

static int enqueue_streaming(rayrs_scene* scene, const FramePlan& p, const FrameDev& d, const WfDev& wf, hipStream_t stream) {
    rayrs_scene::Pool& pl = scene->frame.pool;
    const RenderDev& rp = d.rp;
    uint32_t* h_live = pl.h_live.as<uint32_t>();
    HIP_TRY(wf_launch_init(wf, (uint32_t)p.live_total, stream));
    HIP_TRY(wf_launch_gen(scene->flat.compact, d.sc, d.cam, rp, wf, p.flat_blocks, stream));  // initial fill; later samples start in hit/miss
    h_live[0] = h_live[1] = (uint32_t)p.live_total;
    // Rounds are enqueued in batches; the live-slot count of batch b is read back while batch b+1 is
    // already queued, so the GPU never waits for the host.  Rounds behind the frame's last one find
    // live_slots == 0 and return at once; batches shrink from 16 rounds to 4 once fewer than an eighth of
    // the slots have work, so that at most 7 such rounds are queued after the end.
    constexpr uint32_t MAX_TIMED = 8192;
    uint32_t it = 0;
    uint32_t batch = 16;
    for (uint32_t b = 0;; b++) {
        for (uint32_t k = 0; k < batch; k++, it++) {
            const bool timed = it < MAX_TIMED;  // (rounds beyond the event pool: rayrs_render_finish extrapolates)
            if (timed) RAYRS_TRY(round_event(pl, it, 0, stream));
            HIP_TRY(wf_launch_trav(scene->flat.compact, rp.count_work != 0u, d.sc, rp, wf, p.trav.blocks, stream));
            if (timed) RAYRS_TRY(round_event(pl, it, 1, stream));
            HIP_TRY(wf_launch_hit(scene->flat.compact, p.eager_light, d.sc, d.cam, rp, wf, p.flat_blocks, stream));
            if (timed) RAYRS_TRY(round_event(pl, it, 2, stream));
            HIP_TRY(wf_launch_miss(scene->flat.compact, p.eager_light, d.sc, d.cam, rp, wf, p.flat_blocks, stream));
            if (timed) {
                RAYRS_TRY(round_event(pl, it, 3, stream));
                pl.timed_rounds = it + 1;
            }
        }
        HIP_TRY(hipMemcpyAsync(&h_live[b & 1u], &wf.ctl->live_slots, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipEventRecord(pl.ev_batch[b & 1u], stream));
        if (b > 0) {
            HIP_TRY(hipEventSynchronize(pl.ev_batch[(b - 1u) & 1u]));
            const uint64_t seen = h_live[(b - 1u) & 1u];
            if (seen == 0u) break;
            batch = seen * 8u < p.live_total ? 4u : 16u;
        }
        if (it > (1u << 26)) {
            set_last_error("path rounds did not terminate");
            return RAYRS_HIP_ERROR;
        }
    }
    scene->frame.rounds = it;
    return RAYRS_OK;
}

// A frame, or a film's pass: the samples sample0 .. sample0 + params->spp - 1 of every pixel of the share, summed per chunk
// of that window.  film == nullptr: the chunk sums are resolved into out_device (rayrs_render_launch, sample0 = 0); else
// they are added to the film's records and out_device is not used.  A film pass with a tile list covers the list's tiles
// only, each from its own sample count (sample0 is not used): the plan -- items, pool, grids -- is sized by the list.
int rayrs::render_enqueue(rayrs_scene* scene, const rayrs_camera* camera, const rayrs_render_params* params, uint32_t sample0,
                                       const FilmPassDev* film, void* out_device, void* hip_stream) {
    RAYRS_GUARDED({
    if (!scene || !camera || !params || (!out_device && !film)) return RAYRS_INVALID_ARG;
    if (scene->device < 0) return RAYRS_NO_DEVICE;
    if (params->spp == 0 || camera->x_pixels == 0 || camera->y_pixels == 0) return RAYRS_INVALID_ARG;
    if (camera->x_pixels > 65535u || camera->y_pixels > 65535u) return RAYRS_UNSUPPORTED;  // TailSlot::pix is 16 + 16 bits
    // a path's bounce count and RNG draw index travel as 16 bits each (15 + 16 in the local pool); a bounce draws at
    // most four numbers (material.rs:579 + :1009-1011 + lib.rs:539), so 8000 bounces stay below 2^15 and 2^16
    if (params->max_bounces > 8000u) return RAYRS_UNSUPPORTED;
    if (params->spp > SLOT_SAMPLE_MASK || sample0 > SLOT_SAMPLE_MASK - params->spp) return RAYRS_UNSUPPORTED;  // a slot's sample cursor has 30 bits
    if (params->tile_ranks == 0 || params->tile_rank >= params->tile_ranks) return RAYRS_INVALID_ARG;
    if (params->out_format != RAYRS_OUT_F32 && params->out_format != RAYRS_OUT_F64) return RAYRS_INVALID_ARG;
    if (params->fast_traversal > 1u) return RAYRS_INVALID_ARG;
    HIP_TRY(hipSetDevice(scene->device));
    hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
    rayrs_scene::Frame& fr = scene->frame;
    HIP_TRY(fr.wait());  // one render in flight per scene: its counters and partial sums are shared

    FramePlan p;
    RAYRS_TRY(plan_frame(frame_inputs(scene, camera, params, sample0, film), p));
    FrameDev d;
    d.sc = make_scene_dev(scene, p.exact);
    d.cam = make_camera_dev(camera);
    d.rp = make_render_dev(scene, params, sample0, p, film, out_device);
    d.is_film = film != nullptr;
    d.film = film ? *film : FilmPassDev{};

    // ---- what the plan needs of the scene's buffers, which only grow (nothing of the route the frame does not take)
    rayrs_scene::Pool& pl = fr.pool;
    HIP_TRY(fr.d_partial.reserve(p.partial_bytes));
    d.rp.partial = fr.d_partial.as<double>();
    HIP_TRY(fr.d_local_light.reserve(p.local_light_bytes));
    HIP_TRY(pl.block.reserve(p.pool_bytes));
    HIP_TRY(pl.d_wave_items.reserve(p.wave_items_bytes));
    HIP_TRY(pl.d_stack_spill.reserve(p.spill_bytes));
    WfDev wf = pool_wf(pl.block, p.np, pl.d_ctl, p.trav.blocks, pl.d_stack_spill);
    wf.n_flat_waves = p.flat_blocks * 4u;
    wf.wave_items = pl.d_wave_items.as<unsigned long long>();

    pl.timed_rounds = 0;
    HIP_TRY(hipMemsetAsync(d.rp.counters, 0, sizeof(Counters), stream));
    HIP_TRY(hipMemsetAsync(d.rp.next_item, 0, sizeof(unsigned long long), stream));
    if (p.use_local) HIP_TRY(hipMemsetAsync(fr.d_local_items.as<>(), 0, LOCAL_MAX_SEGMENTS * sizeof(unsigned long long), stream));
    HIP_TRY(hipEventRecord(fr.ev[0], stream));
    fr.rounds = 0;
    fr.taken = {p.use_local, p.exact, p.hot_group};
    if (p.total_items > 0) RAYRS_TRY(p.use_local ? enqueue_local(scene, p, d, stream) : enqueue_streaming(scene, p, d, wf, stream));
    HIP_TRY(hipEventRecord(fr.ev[1], stream));
    if (!p.use_local) HIP_TRY(d.is_film ? launch_film_accumulate(d.cam, d.rp, d.film, 0u, d.rp.n_local_tiles, stream) : launch_resolve(d.cam, d.rp, 0u, d.rp.n_local_tiles, stream));
    HIP_TRY(hipEventRecord(fr.ev[2], stream));
    fr.last_stream = stream;
    fr.pending = true;
    return RAYRS_OK;
    })
}

int rayrs::render_finish(rayrs_scene* scene, rayrs_render_stats* stats) {
    if (scene->device < 0) return RAYRS_NO_DEVICE;
    rayrs_scene::Frame& fr = scene->frame;
    if (!fr.pending) return RAYRS_INVALID_ARG;
    HIP_TRY(hipSetDevice(scene->device));
    HIP_TRY(hipEventSynchronize(fr.ev[2]));
    fr.pending = false;
    if (stats) {
        Counters c;
        HIP_TRY(fr.d_counters.download(&c, sizeof(c)));
        std::memset(stats, 0, sizeof(*stats));
#define RAYRS_COPY(name) stats->name = c.name;
        RAYRS_WORK_COUNTERS(RAYRS_COPY)
#undef RAYRS_COPY
        for (int k = 0; k < 8; k++) stats->surface_hits[k] = c.surface_hits[k];
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, fr.ev[0], fr.ev[1]));
        stats->trace_ms = ms;
        HIP_TRY(hipEventElapsedTime(&ms, fr.ev[0], fr.ev[2]));
        stats->total_ms = ms;
        const uint32_t timed_rounds = fr.pool.timed_rounds;
        double t = 0.0, h = 0.0, m = 0.0;
        for (uint32_t r = 0; r < timed_rounds; r++) {
            float k[3];
            RAYRS_TRY(round_ms(scene, r, k));
            t += k[0], h += k[1], m += k[2];
        }
        // rounds beyond the event pool (very long renders) are extrapolated from the timed ones
        if (timed_rounds && fr.rounds > timed_rounds) {
            const double f = (double)fr.rounds / (double)timed_rounds;
            t *= f, h *= f, m *= f;
        }
        stats->kernel_ms = t;
        stats->hit_ms = h, stats->miss_ms = m;
        stats->local_pool = fr.taken.use_local ? 1u : 0u;
        stats->exact_walk = (fr.taken.exact || fr.taken.use_local) ? 1u : 0u;
        stats->hot_group = fr.taken.hot_group ? 1u : 0u;
        stats->kernel_launches = (uint64_t)fr.rounds;
    }
    return RAYRS_OK;
}
