// film_abi.cpp -- the progressive film of include/rayrs_hip.h (rayrs_film_*): a film's lifetime, a pass as a render of a
// sample window whose chunk sums go to the film's records (render.cpp render_enqueue, film.hip), the frame and the status
// read from the records, and the checkpoint image.  A direct-lit film (DIRECT-LIT FILMS) differs in who makes a pass's chunk
// sums: film_direct.hip's kernels on the scene's radiance scratch, launch by launch (film_pass_lit); with a mesh-light group
// of N >= 1 triangles (MESH-LIT FILMS AND BAKES) film_mesh.hip's.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "../../include/rayrs_hip.h"
#include "denoise_host.hpp"
#include "features_host.hpp"
#include "film.h"
#include "film_direct_kernels.h"
#include "film_host.hpp"
#include "passes_mesh_kernels.h"
#include "radiance_lit_host.hpp"
#include "scene_internal.hpp"

using namespace rayrs;

namespace {
// The checkpoint image: this header, then the film's records as they lie on the device (film.h), then N_t of every tile
// of the frame, row-major, 4 bytes each (version 2; version 1 had no per-tile counts).
constexpr uint32_t STATE_MAGIC = 0x4d4c4652u;  // "RFLM"
constexpr uint32_t STATE_VERSION = 2;
struct StateHeader {
    uint32_t magic, version;
    uint32_t x_pixels, y_pixels;
    uint32_t sample_chunk, max_bounces;
    uint64_t seed;
    uint32_t tile_rank, tile_ranks;
    uint32_t fast_traversal, closed;
    uint64_t samples, full_chunks, rays, paths;  // samples: the largest N_t
    uint64_t record_bytes;
};
static_assert(sizeof(StateHeader) == 88, "StateHeader");
constexpr size_t STAGE_BYTES = 8u << 20;  // pinned staging of state_get / state_set, copied through in pieces
}  // namespace

struct rayrs_film {
    rayrs_scene* scene = nullptr;  // not owned
    rayrs_camera camera = {};
    rayrs_film_params prm = {};    // as given, defaults filled in
    TileShare share = {};          // the film's tiles of the frame's (layout.h)
    // samples: N of a uniform film; once the tiles differ, the largest N_t as last read from the device (film_max_samples)
    uint64_t samples = 0, rays = 0, paths = 0;
    bool uniform = true;  // every tile of the share holds `samples` samples (no adaptive pass has left any out yet)
    bool closed = false;
    DevBuf d_rec;     // film.h: 40 bytes per pixel of the frame's tiles
    DevBuf d_tile_n;  // N_t: one word per tile of the frame, 0 outside the share
    DevBuf d_flags;   // an adaptive pass: one word per tile of the share (film_select_kernel) ...
    DevBuf d_list;    // ... and the list made of them, one TileRef per tile of the share at most
    DevBuf d_select;  // one FilmSelect
    PinnedBuf h_word; // one word of it, read back (film_select)
    DevBuf d_counts;  // one FilmCounts
    DevBuf d_out;     // the frame rayrs_film_read copies out, grown on demand
    PinnedBuf h_stage;
    bool has_stage = false;
    // The features of the film's view (rayrs_film_features, rayrs_film_denoise), kept on the device under the sample count
    // they were made with: they depend on the film's camera, seed, share and walk, never on the samples it holds.  Not
    // part of the checkpoint image.
    FeatureBufs feat;
    uint32_t feat_samples = 0;  // 0 = none yet
    DevBuf d_var;               // the noise plane (rayrs_film_noise, rayrs_film_denoise_guided), grown on demand
    DenoiseBufs filter;         // what either filter works in
    // DIRECT-LIT FILMS: the film's passes are direct-lit (rayrs_film_create_direct), with the sky among the lights
    // (rayrs_film_create_sky); the list as given, fixed for the film's life.  Not part of the checkpoint image.
    bool lit = false, sky = false;
    std::vector<uint32_t> lights;
    // MESH-LIT FILMS AND BAKES: the group of rayrs_film_create_mesh, borrowed (it outlives the film); null or empty: none
    const rayrs_mesh_lights* mesh = nullptr;
    bool grouped() const { return mesh && mesh->n != 0u; }
    DevBuf d_lit_counts;  // one FilmDirectCounts, read once per pass
    Event lit_ev[2];      // around a pass's launches
    LitCall lit_call(uint32_t n) const {
        return LitCall{LIT_START_PIXEL, n, prm.max_bounces, prm.sample_chunk, 0.0, prm.seed, 0u, prm.fast_traversal, lights.data(),
                       (uint32_t)lights.size(), true, sky, mesh};
    }
    // a lit pass of n samples is too long: a tile's items of one pass do not fit one launch
    bool lit_pass_too_long(uint32_t n) const { return lit && ((uint64_t)n + prm.sample_chunk - 1u) / prm.sample_chunk * 64u > RADIANCE_LAUNCH_ITEMS; }
    size_t record_bytes() const { return n_tiles() * FILM_TILE_DOUBLES * sizeof(double); }
    size_t n_tiles() const { return (size_t)share.tiles_x * share.tiles_y; }
    size_t count_bytes() const { return n_tiles() * sizeof(uint32_t); }
    uint64_t full_chunks() const { return samples / prm.sample_chunk; }
    StateHeader header() const {
        StateHeader h;
        std::memset(&h, 0, sizeof(h));
        h.magic = STATE_MAGIC, h.version = STATE_VERSION;
        h.x_pixels = camera.x_pixels, h.y_pixels = camera.y_pixels;
        h.sample_chunk = prm.sample_chunk, h.max_bounces = prm.max_bounces, h.seed = prm.seed;
        h.tile_rank = prm.tile_rank, h.tile_ranks = prm.tile_ranks, h.fast_traversal = prm.fast_traversal;
        h.closed = closed ? 1u : 0u;
        h.samples = samples, h.full_chunks = full_chunks(), h.rays = rays, h.paths = paths;
        h.record_bytes = record_bytes();
        return h;
    }
};

// a film's calls run on the scene's device, behind whatever the scene still has in flight
static int film_enter(rayrs_film* f) { return scene_settle(f->scene); }

// Makes the list of a pass over some of the share's tiles (film.hip): those an adaptive pass of n samples selects at tau
// under the cap, or all of them.  One word of the result comes back through the film's pinned word -- the list's length,
// which the pass is planned from, or (all) the largest N_t, which bounds the pass -- and that copy is the only wait.
static int film_select(rayrs_film* f, uint32_t n, uint32_t cap, double tau, bool all, uint32_t* word) {
    HIP_TRY(f->d_flags.reserve((size_t)f->share.n_local_tiles * sizeof(uint32_t)));
    HIP_TRY(f->d_list.reserve((size_t)f->share.n_local_tiles * sizeof(TileRef)));
    const CameraDev cam = make_camera_dev(&f->camera);
    FilmSelect* sel = f->d_select.as<FilmSelect>();
    HIP_TRY(launch_film_select(cam, f->share, f->d_rec.as<double>(), f->d_tile_n.as<uint32_t>(), f->prm.sample_chunk, n, cap, tau * tau,
                               all ? 1u : 0u, f->d_flags.as<uint32_t>(), f->d_list.as<TileRef>(), sel, nullptr));
    uint32_t* h_word = f->h_word.as<uint32_t>();
    HIP_TRY(hipMemcpyAsync(h_word, all ? &sel->max_samples : &sel->n_active, sizeof(uint32_t), hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    *word = *h_word;
    return RAYRS_OK;
}

// One pass of n samples: over the list film_select has just made (n_list tiles, each from its own N_t), or, n_list == 0,
// over the whole share of a uniform film from `samples`.
static int film_pass_lit(rayrs_film* film, uint32_t n, uint32_t n_list, rayrs_render_stats* st);
static int film_pass(rayrs_film* film, uint32_t n, uint32_t n_list, rayrs_render_stats* st) {
    if (film->lit) return film_pass_lit(film, n, n_list, st);
    const uint32_t c = film->prm.sample_chunk;
    rayrs_render_params p;
    std::memset(&p, 0, sizeof(p));
    p.spp = n;  // the pass's window: its chunks are chunks N/c .. of the one-shot frame, N being a multiple of c
    p.max_bounces = film->prm.max_bounces;
    p.seed = film->prm.seed;
    p.sample_chunk = c;  // (c >= n: the window is one chunk, full if n == c)
    p.tile_rank = film->prm.tile_rank, p.tile_ranks = film->prm.tile_ranks;
    p.out_format = RAYRS_OUT_F64;
    p.fast_traversal = film->prm.fast_traversal;
    FilmPassDev fp;
    std::memset(&fp, 0, sizeof(fp));
    fp.rec = film->d_rec.as<double>();
    fp.first = film->samples == 0 ? 1u : 0u;
    fp.full_chunks = n / c;
    fp.tile_n = film->d_tile_n.as<uint32_t>();
    fp.list = n_list ? film->d_list.as<TileRef>() : nullptr;
    fp.n_list = n_list;
    // the accumulate kernel follows the pass's path rounds on the same stream: no host round trip in between
    RAYRS_TRY(render_enqueue(film->scene, &film->camera, &p, n_list ? 0u : (uint32_t)film->samples, &fp, nullptr, nullptr));
    RAYRS_TRY(rayrs_render_finish(film->scene, st));
    film->rays += st->rays, film->paths += st->paths;
    return RAYRS_OK;
}

// The same pass of a direct-lit film.  Whole tiles, as many as fit RADIANCE_LAUNCH_ITEMS items, per launch of the direct, the
// sky or (a group of N >= 1 triangles) the mesh wave on the scene's radiance scratch (the queries' ordering rule,
// radiance_lit_abi.cpp lit_scratch_begin); behind each
// launch, on the same stream, its counts and film_accumulate_kernel over its tile range, as behind a segment of a plain pass.
// The host waits once, for the pass's two counters.
static int film_pass_lit(rayrs_film* film, uint32_t n, uint32_t n_list, rayrs_render_stats* st) {
    rayrs_scene* scene = film->scene;
    const uint32_t c = film->prm.sample_chunk;
    const LitCall call = film->lit_call(n);
    const LightsDev lights = lights_resolve(scene, call);
    const LightSlotsDev slots = direct_slots(scene, call);
    SkyDev sky;
    std::memset(&sky, 0, sizeof(sky));
    if (film->sky) RAYRS_TRY(sky_device_table(scene, &sky));
    MeshDev mesh;
    std::memset(&mesh, 0, sizeof(mesh));
    const bool grouped = film->grouped();
    if (grouped) RAYRS_TRY(mesh_device_table(film->mesh, &mesh));  // (uploaded by the handle's first call, then kept)
    const FrameWalk walk = frame_walk(scene, &film->camera, film->prm.fast_traversal);  // the walk a render with these settings takes
    const SceneDev sc = make_scene_dev(scene, walk.exact || walk.use_local);
    const CameraDev cam = make_camera_dev(&film->camera);
    const hipStream_t stream = nullptr;
    RadianceDev rd;
    std::memset(&rd, 0, sizeof(rd));
    RAYRS_TRY(lit_scratch_begin(scene, sc, stream, &rd));
    rd.samples = n, rd.max_bounces = film->prm.max_bounces, rd.seed = film->prm.seed;
    rd.chunk = c, rd.chunks = (n + c - 1u) / c;  // (n and c are below 2^30)
    const uint32_t n_tiles = n_list ? n_list : film->share.n_local_tiles;
    FilmStartDev fs;
    std::memset(&fs, 0, sizeof(fs));
    fs.share = film->share, fs.share.n_local_tiles = n_tiles;
    fs.tile_list = n_list ? film->d_list.as<TileRef>() : nullptr;
    fs.sample0 = n_list ? 0u : (uint32_t)film->samples, fs.spp = n;
    RenderDev rp;  // what film_accumulate_kernel reads of it
    std::memset(&rp, 0, sizeof(rp));
    rp.spp = n, rp.sample0 = fs.sample0, rp.max_bounces = rd.max_bounces, rp.seed = rd.seed;
    rp.chunk = c, rp.nchunks = rd.chunks;
    rp.tile_rank = fs.share.tile_rank, rp.tile_ranks = fs.share.tile_ranks;
    rp.tiles_x = fs.share.tiles_x, rp.tiles_y = fs.share.tiles_y, rp.n_local_tiles = n_tiles;
    rp.total_items = (uint64_t)n_tiles * rp.nchunks * 64u;
    rp.inv_nchunks = 1.0 / (double)rp.nchunks, rp.inv_tiles_x = 1.0 / (double)rp.tiles_x;
    rp.out_format = RAYRS_OUT_F64;
    rp.partial = rd.partial;
    rp.tile_list = fs.tile_list;
    FilmPassDev fp;
    std::memset(&fp, 0, sizeof(fp));
    fp.rec = film->d_rec.as<double>();
    fp.first = film->samples == 0 ? 1u : 0u;
    fp.full_chunks = n / c;
    fp.tile_n = film->d_tile_n.as<uint32_t>();
    fp.list = fs.tile_list, fp.n_list = n_list;
    FilmDirectCounts* counts = film->d_lit_counts.as<FilmDirectCounts>();
    HIP_TRY(hipMemsetAsync(counts, 0, sizeof(FilmDirectCounts), stream));
    HIP_TRY(hipEventRecord(film->lit_ev[0], stream));
    const uint32_t per_launch = (uint32_t)(RADIANCE_LAUNCH_ITEMS / (64u * (uint64_t)rd.chunks));  // (>= 1: lit_pass_too_long)
    for (uint32_t lt0 = 0; lt0 < n_tiles; lt0 += per_launch) {
        const uint32_t n_lt = n_tiles - lt0 < per_launch ? n_tiles - lt0 : per_launch;
        rd.n = n_lt * 64u;
        fs.lt0 = lt0;
        rp.partial_item0 = (uint64_t)lt0 * rp.nchunks * 64u;
        if (rd.max_bounces == 0u) {  // the loop runs no turn: +0 and no query, whatever the scene
            HIP_TRY(hipMemsetAsync(rd.partial, 0, (size_t)rd.n * rd.chunks * 3u * sizeof(double), stream));
        } else {
            HIP_TRY(hipMemsetAsync(rd.cursor, 0, sizeof(unsigned long long), stream));
            if (grouped) HIP_TRY(launch_film_mesh(scene->flat.compact, sc, rd, fs, lights, slots, mesh, sky, film->sky, cam, scene->cu_count, stream));
            else HIP_TRY(launch_film_direct(scene->flat.compact, sc, rd, fs, lights, slots, film->sky ? &sky : nullptr, cam, scene->cu_count, stream));
        }
        HIP_TRY(launch_film_direct_count(rd, fs, cam, rd.max_bounces != 0u ? 1u : 0u, counts, stream));
        HIP_TRY(launch_film_accumulate(cam, rp, fp, lt0, n_lt, stream));
    }
    HIP_TRY(hipEventRecord(film->lit_ev[1], stream));
    RAYRS_TRY(lit_scratch_end(scene, stream));
    FilmDirectCounts got;
    HIP_TRY(film->d_lit_counts.download(&got, sizeof(got)));  // (the pass's one wait)
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, film->lit_ev[0], film->lit_ev[1]));
    std::memset(st, 0, sizeof(*st));
    st->rays = got.queries, st->paths = got.pixels * n;
    st->exact_walk = sc.exact;
    st->kernel_ms = ms, st->total_ms = ms;  // the waves' launches, and all of the pass's kernels: one HIP-event interval
    film->rays += st->rays, film->paths += st->paths;
    return RAYRS_OK;
}

static int film_stage(rayrs_film* f) {
    if (!f->has_stage) {
        HIP_TRY(f->h_stage.alloc(STAGE_BYTES));
        f->has_stage = true;
    }
    return RAYRS_OK;
}

// rayrs_film_create (lit == nullptr), or a direct-lit film of lit's list: its refusals join the plain film's, group by group.
static int film_create(rayrs_scene* scene, const rayrs_camera* camera, const rayrs_film_params* params, const LitCall* lit, rayrs_film** out) {
    if (!scene || !camera || !params || !out) return RAYRS_INVALID_ARG;
    *out = nullptr;
    rayrs_film_params prm = *params;
    if (prm.sample_chunk == 0) prm.sample_chunk = 4;
    if (prm.tile_ranks == 0 && prm.tile_rank == 0) prm.tile_ranks = 1;
    if (camera->x_pixels == 0 || camera->y_pixels == 0) return RAYRS_INVALID_ARG;
    if (prm.tile_ranks == 0 || prm.tile_rank >= prm.tile_ranks || prm.fast_traversal > 1u || prm.pad != 0u) return RAYRS_INVALID_ARG;
    if (lit) RAYRS_TRY(lit_list_invalid(scene, *lit));
    if (lit && lit->mesh && lit->mesh->scene != scene) return RAYRS_INVALID_ARG;
    if (lit && lit->mesh && lit->mesh->tree) return RAYRS_UNSUPPORTED;  // LIGHT TREE: the passes have no kernel that descends a tree
    if (camera->x_pixels > 65535u || camera->y_pixels > 65535u) return RAYRS_UNSUPPORTED;
    if (prm.max_bounces > 8000u) return RAYRS_UNSUPPORTED;
    if (prm.sample_chunk > SLOT_SAMPLE_MASK) return RAYRS_UNSUPPORTED;  // not one full chunk fits the 30-bit sample cursor
    if (lit) {
        RAYRS_TRY(lit_list_unsupported(scene, *lit));
        // (an item is one chunk of at most 2 * max_bounces + 1 queries a sample, counted in 32 bits)
        if ((uint64_t)prm.sample_chunk * (2ull * prm.max_bounces + 1u) >= (1ull << 32)) return RAYRS_UNSUPPORTED;
    }
    if (scene->device < 0) return RAYRS_NO_DEVICE;
    std::unique_ptr<rayrs_film> f(new rayrs_film());
    f->scene = scene;
    f->camera = *camera;
    f->prm = prm;
    f->share = tile_share(camera->x_pixels, camera->y_pixels, prm.tile_rank, prm.tile_ranks);
    HIP_TRY(hipSetDevice(scene->device));
    HIP_TRY(f->d_rec.reserve(f->record_bytes()));
    HIP_TRY(hipMemset(f->d_rec.as<>(), 0, f->record_bytes()));
    HIP_TRY(f->d_tile_n.reserve(f->count_bytes()));
    HIP_TRY(hipMemset(f->d_tile_n.as<>(), 0, f->count_bytes()));
    HIP_TRY(f->d_select.reserve(sizeof(FilmSelect)));
    HIP_TRY(f->h_word.alloc(sizeof(uint32_t)));
    HIP_TRY(f->d_counts.reserve(sizeof(FilmCounts)));
    if (lit) {
        f->lit = true, f->sky = lit->sky, f->mesh = lit->mesh;
        f->lights.assign(lit->lights, lit->lights + lit->n_lights);
        HIP_TRY(f->d_lit_counts.reserve(sizeof(FilmDirectCounts)));
        HIP_TRY(f->lit_ev[0].create());
        HIP_TRY(f->lit_ev[1].create());
    }
    *out = f.release();
    return RAYRS_OK;
}

// the list of a direct-lit film's creation as the light-list entry points describe a call (the film's own settings join it later)
static LitCall film_list(const uint32_t* lights, uint32_t n_lights, bool sky, const rayrs_mesh_lights* mesh = nullptr) {
    return LitCall{LIT_START_PIXEL, 0u, 0u, 0u, 0.0, 0u, 0u, 0u, lights, n_lights, true, sky, mesh};
}

extern "C" {

int rayrs_film_create(rayrs_scene* scene, const rayrs_camera* camera, const rayrs_film_params* params, rayrs_film** out) {
    RAYRS_GUARDED({ return film_create(scene, camera, params, nullptr, out); })
}

int rayrs_film_create_direct(rayrs_scene* scene, const rayrs_camera* camera, const rayrs_film_params* params, const uint32_t* lights,
                             uint32_t n_lights, rayrs_film** out) {
    RAYRS_GUARDED({
    const LitCall lit = film_list(lights, n_lights, false);
    return film_create(scene, camera, params, &lit, out);
    })
}

int rayrs_film_create_sky(rayrs_scene* scene, const rayrs_camera* camera, const rayrs_film_params* params, const uint32_t* lights,
                          uint32_t n_lights, rayrs_film** out) {
    RAYRS_GUARDED({
    const LitCall lit = film_list(lights, n_lights, true);
    return film_create(scene, camera, params, &lit, out);
    })
}

int rayrs_film_create_mesh(rayrs_scene* scene, const rayrs_camera* camera, const rayrs_film_params* params, const uint32_t* lights,
                           uint32_t n_lights, const rayrs_mesh_lights* mesh, uint32_t sky, rayrs_film** out) {
    RAYRS_GUARDED({
    if (out) *out = nullptr;
    if (sky > 1u) return RAYRS_INVALID_ARG;  // (of that group whatever else is asked, as MESH LIGHTS' entry points have it)
    const LitCall lit = film_list(lights, n_lights, sky == 1u, mesh);
    return film_create(scene, camera, params, &lit, out);
    })
}

void rayrs_film_destroy(rayrs_film* film) {
    if (!film) return;
    // (the scene outlives its films: the header's rule)
    if (film->scene && film->scene->device >= 0) (void)hipSetDevice(film->scene->device);
    delete film;
}

int rayrs_film_render(rayrs_film* film, uint32_t n, rayrs_render_stats* pass_stats) {
    RAYRS_GUARDED({
    if (!film || n == 0 || film->closed) return RAYRS_INVALID_ARG;
    const uint32_t c = film->prm.sample_chunk;
    if (n > SLOT_SAMPLE_MASK || film->lit_pass_too_long(n)) return RAYRS_UNSUPPORTED;
    if (film->uniform && (film->samples > SLOT_SAMPLE_MASK || n > SLOT_SAMPLE_MASK - (uint32_t)film->samples)) return RAYRS_UNSUPPORTED;
    RAYRS_TRY(film_enter(film));
    uint32_t n_list = 0;
    if (!film->uniform) {  // every tile of the share from its own N_t: a pass over the list of them all
        uint32_t most = 0;
        RAYRS_TRY(film_select(film, n, 0u, 0.0, true, &most));
        film->samples = most;
        if (most > SLOT_SAMPLE_MASK || n > SLOT_SAMPLE_MASK - most) return RAYRS_UNSUPPORTED;
        n_list = film->share.n_local_tiles;
    }
    rayrs_render_stats st;
    RAYRS_TRY(film_pass(film, n, n_list, &st));
    film->samples += n;
    if (n % c != 0u) film->closed = true;
    if (pass_stats) *pass_stats = st;
    return RAYRS_OK;
    })
}

int rayrs_film_render_adaptive(rayrs_film* film, uint32_t n, double tau, uint32_t max_tile_samples, uint64_t* active_tiles,
                               rayrs_render_stats* pass_stats) {
    RAYRS_GUARDED({
    if (!film || n == 0 || film->closed || !(tau >= 0.0) || !std::isfinite(tau)) return RAYRS_INVALID_ARG;
    if (n % film->prm.sample_chunk != 0u) return RAYRS_INVALID_ARG;
    if (film->lit_pass_too_long(n)) return RAYRS_UNSUPPORTED;
    RAYRS_TRY(film_enter(film));
    const uint32_t cap = max_tile_samples != 0u && max_tile_samples < SLOT_SAMPLE_MASK ? max_tile_samples : SLOT_SAMPLE_MASK;
    uint32_t active = 0;
    RAYRS_TRY(film_select(film, n, cap, tau, false, &active));
    rayrs_render_stats st;
    std::memset(&st, 0, sizeof(st));
    if (active != 0u) {
        RAYRS_TRY(film_pass(film, n, active, &st));
        if (film->uniform && active == film->share.n_local_tiles) film->samples += n;  // every tile went on
        else film->uniform = false;
    }
    if (active_tiles) *active_tiles = active;
    if (pass_stats) *pass_stats = st;
    return RAYRS_OK;
    })
}

uint64_t rayrs_film_tile_samples(rayrs_film* film, uint32_t* out, uint64_t cap) {
    if (!film) return 0;
    const uint64_t n = film->n_tiles();
    const uint64_t take = cap < n ? cap : n;
    if (out && take) {
        if (film_enter(film) != RAYRS_OK) return 0;
        if (film->d_tile_n.download(out, (size_t)take * sizeof(uint32_t)) != hipSuccess) return 0;
    }
    return n;
}

int rayrs_film_read(rayrs_film* film, uint32_t out_format, void* out_host) {
    RAYRS_GUARDED({
    if (!film || !out_host || film->samples == 0) return RAYRS_INVALID_ARG;
    if (out_format != RAYRS_OUT_F32 && out_format != RAYRS_OUT_F64) return RAYRS_INVALID_ARG;
    RAYRS_TRY(film_enter(film));
    const size_t bytes = frame_bytes(film->camera.x_pixels, film->camera.y_pixels, out_format);
    HIP_TRY(film->d_out.reserve(bytes));
    const CameraDev cam = make_camera_dev(&film->camera);
    HIP_TRY(launch_film_read(cam, film->share.tiles_x, film->d_rec.as<double>(), film->d_tile_n.as<uint32_t>(), out_format,
                             film->d_out.as<>(), nullptr));
    HIP_TRY(film->d_out.download(out_host, bytes));
    return RAYRS_OK;
    })
}

int rayrs_film_status_get(rayrs_film* film, double tau, rayrs_film_status* out) {
    RAYRS_GUARDED({
    if (!film || !out || !(tau >= 0.0) || !std::isfinite(tau)) return RAYRS_INVALID_ARG;
    RAYRS_TRY(film_enter(film));
    const CameraDev cam = make_camera_dev(&film->camera);
    HIP_TRY(hipMemsetAsync(film->d_counts.as<>(), 0, sizeof(FilmCounts), nullptr));
    HIP_TRY(launch_film_status(cam, film->share, film->d_rec.as<double>(), film->d_tile_n.as<uint32_t>(), film->prm.sample_chunk, tau * tau,
                               film->d_counts.as<FilmCounts>(), nullptr));
    FilmCounts c;
    HIP_TRY(film->d_counts.download(&c, sizeof(c)));
    if (!film->uniform) film->samples = c.max_samples;  // the largest N_t
    std::memset(out, 0, sizeof(*out));
    out->samples = film->samples, out->full_chunks = film->full_chunks();
    out->rays = film->rays, out->paths = film->paths;
    out->nan_pixels = c.nan_pixels, out->neg_pixels = c.neg_pixels;
    out->unconverged = c.unconverged, out->nonfinite = c.nonfinite;
    out->closed = film->closed ? 1u : 0u;
    return RAYRS_OK;
    })
}

// the film's features for `samples` samples, made now unless the film holds them
static int film_features(rayrs_film* f, uint32_t samples) {
    if (f->feat_samples == samples) return RAYRS_OK;
    f->feat_samples = 0;
    RAYRS_TRY(features_run(f->scene, &f->camera, samples, f->prm.seed, f->prm.tile_rank, f->prm.tile_ranks, f->prm.fast_traversal,
                           f->feat));
    f->feat_samples = samples;
    return RAYRS_OK;
}

int rayrs_film_features(rayrs_film* film, uint32_t samples, double* normal, double* albedo, double* depth, double* coverage,
                        uint32_t* object) {
    RAYRS_GUARDED({
    if (!film) return RAYRS_INVALID_ARG;
    RAYRS_TRY(features_check(&film->camera, samples, film->prm.tile_rank, film->prm.tile_ranks, film->prm.fast_traversal));
    RAYRS_TRY(film_enter(film));
    RAYRS_TRY(film_features(film, samples));
    RAYRS_TRY(features_download(film->scene, &film->camera, film->feat, normal, albedo, depth, coverage, object));
    return RAYRS_OK;
    })
}

// the noise plane of the film as it stands into d_var (include/rayrs_hip.h NOISE PLANE); pixels outside the share read +0
static int film_noise_plane(rayrs_film* f) {
    const size_t bytes = (size_t)f->camera.x_pixels * f->camera.y_pixels * sizeof(double);
    HIP_TRY(f->d_var.reserve(bytes));
    HIP_TRY(hipMemsetAsync(f->d_var.as<>(), 0, bytes, nullptr));
    FilmNoiseDev n;
    std::memset(&n, 0, sizeof(n));
    n.rec = f->d_rec.as<double>(), n.tile_n = f->d_tile_n.as<uint32_t>();
    n.variance = f->d_var.as<double>();
    n.w = f->camera.x_pixels, n.h = f->camera.y_pixels;
    n.share = f->share, n.c = f->prm.sample_chunk;
    HIP_TRY(launch_film_noise(n, nullptr));
    return RAYRS_OK;
}

int rayrs_film_noise(rayrs_film* film, double* variance_host) {
    RAYRS_GUARDED({
    if (!film || !variance_host || film->samples == 0) return RAYRS_INVALID_ARG;
    RAYRS_TRY(film_enter(film));
    RAYRS_TRY(film_noise_plane(film));
    HIP_TRY(film->d_var.download(variance_host, (size_t)film->camera.x_pixels * film->camera.y_pixels * sizeof(double)));
    return RAYRS_OK;
    })
}

// Both of the film's filters: the refusals, the film's features, the frame rayrs_film_read(RAYRS_OUT_F64) returns left in
// d_out and, guided, the plane rayrs_film_noise returns in d_var; then the levels, and the result copied out.
static int film_denoise(rayrs_film* film, bool guided, uint32_t feature_samples, uint32_t levels, double kn, double ka, double kz,
                        double k, uint32_t out_format, void* out_host, double* out_variance) {
    if (!film || !out_host || film->samples == 0) return RAYRS_INVALID_ARG;
    if (out_format != RAYRS_OUT_F32 && out_format != RAYRS_OUT_F64) return RAYRS_INVALID_ARG;
    if (film->prm.tile_ranks > 1u) return RAYRS_INVALID_ARG;  // the filter needs a pixel's neighbours
    RAYRS_TRY(denoise_check(levels, kn, ka, kz, k));  // the same rule for kv as for kc
    RAYRS_TRY(features_check(&film->camera, feature_samples, film->prm.tile_rank, film->prm.tile_ranks, film->prm.fast_traversal));
    RAYRS_TRY(film_enter(film));
    RAYRS_TRY(film_features(film, feature_samples));
    const uint32_t w = film->camera.x_pixels, h = film->camera.y_pixels;
    HIP_TRY(film->d_out.reserve(frame_bytes(w, h, RAYRS_OUT_F64)));
    const CameraDev cam = make_camera_dev(&film->camera);
    HIP_TRY(launch_film_read(cam, film->share.tiles_x, film->d_rec.as<double>(), film->d_tile_n.as<uint32_t>(), RAYRS_OUT_F64,
                             film->d_out.as<>(), nullptr));
    if (guided) RAYRS_TRY(film_noise_plane(film));
    const DenoiseIn in{w, h, film->d_out.as<double>(), guided ? film->d_var.as<double>() : nullptr, film->feat.normal.as<double>(),
                       film->feat.albedo.as<double>(), film->feat.depth.as<double>()};
    const void* result = nullptr;
    RAYRS_TRY(denoise_run(in, levels, kn, ka, kz, k, out_format, out_variance != nullptr, film->filter, &result));
    HIP_TRY(hipMemcpy(out_host, result, frame_bytes(w, h, out_format), hipMemcpyDeviceToHost));
    if (out_variance) HIP_TRY(film->filter.variance.download(out_variance, (size_t)w * h * sizeof(double)));
    return RAYRS_OK;
}

int rayrs_film_denoise(rayrs_film* film, uint32_t feature_samples, uint32_t levels, double kn, double ka, double kz, double kc,
                       uint32_t out_format, void* out_host) {
    RAYRS_GUARDED({ return film_denoise(film, false, feature_samples, levels, kn, ka, kz, kc, out_format, out_host, nullptr); })
}

int rayrs_film_denoise_guided(rayrs_film* film, uint32_t feature_samples, uint32_t levels, double kn, double ka, double kz, double kv,
                              uint32_t out_format, void* out_host, double* out_variance) {
    RAYRS_GUARDED({ return film_denoise(film, true, feature_samples, levels, kn, ka, kz, kv, out_format, out_host, out_variance); })
}

uint64_t rayrs_film_state_bytes(const rayrs_film* film) {
    return film ? sizeof(StateHeader) + film->record_bytes() + film->count_bytes() : 0;
}

int rayrs_film_state_get(rayrs_film* film, void* out_host, uint64_t cap) {
    RAYRS_GUARDED({
    if (!film || !out_host || cap < rayrs_film_state_bytes(film)) return RAYRS_INVALID_ARG;
    RAYRS_TRY(film_enter(film));
    RAYRS_TRY(film_stage(film));
    uint8_t* counts = static_cast<uint8_t*>(out_host) + sizeof(StateHeader) + film->record_bytes();
    HIP_TRY(film->d_tile_n.download(counts, film->count_bytes()));
    if (!film->uniform) {
        uint32_t most = 0;
        for (size_t t = 0; t < film->n_tiles(); t++) {
            uint32_t n_t;
            std::memcpy(&n_t, counts + t * sizeof(uint32_t), sizeof(n_t));
            most = n_t > most ? n_t : most;
        }
        film->samples = most;
    }
    const StateHeader h = film->header();
    uint8_t* dst = static_cast<uint8_t*>(out_host);
    std::memcpy(dst, &h, sizeof(h));
    dst += sizeof(h);
    const uint8_t* src = film->d_rec.as<uint8_t>();
    for (size_t at = 0, total = film->record_bytes(); at < total; at += STAGE_BYTES) {
        const size_t piece = total - at < STAGE_BYTES ? total - at : STAGE_BYTES;
        HIP_TRY(hipMemcpyAsync(film->h_stage.as<void>(), src + at, piece, hipMemcpyDeviceToHost, nullptr));
        HIP_TRY(hipStreamSynchronize(nullptr));
        std::memcpy(dst + at, film->h_stage.as<void>(), piece);
    }
    return RAYRS_OK;
    })
}

int rayrs_film_state_set(rayrs_film* film, const void* in_host, uint64_t bytes) {
    RAYRS_GUARDED({
    if (!film || !in_host || bytes < sizeof(StateHeader)) return RAYRS_INVALID_ARG;
    StateHeader h;
    std::memcpy(&h, in_host, sizeof(h));
    const StateHeader mine = film->header();
    if (h.magic != STATE_MAGIC || h.version != STATE_VERSION) return RAYRS_INVALID_ARG;
    if (h.x_pixels != mine.x_pixels || h.y_pixels != mine.y_pixels || h.sample_chunk != mine.sample_chunk ||
        h.max_bounces != mine.max_bounces || h.seed != mine.seed || h.tile_rank != mine.tile_rank ||
        h.tile_ranks != mine.tile_ranks || h.fast_traversal != mine.fast_traversal)
        return RAYRS_INVALID_ARG;
    if (h.record_bytes != mine.record_bytes || bytes != rayrs_film_state_bytes(film)) return RAYRS_INVALID_ARG;
    // counters that no sequence of passes leaves behind: not this library's image
    const uint64_t c = mine.sample_chunk;
    if (h.closed > 1u || h.samples > SLOT_SAMPLE_MASK || h.full_chunks != h.samples / c || (h.closed == 0u) != (h.samples % c == 0u))
        return RAYRS_INVALID_ARG;
    // ... and per-tile counts that none leaves: nothing outside the share; in an open film whole chunks, in a closed one
    // the same short chunk everywhere; the largest is the header's
    std::vector<uint32_t> counts(film->n_tiles());
    std::memcpy(counts.data(), static_cast<const uint8_t*>(in_host) + sizeof(h) + h.record_bytes, film->count_bytes());
    uint32_t most = 0;
    bool same = true;
    for (size_t t = 0; t < counts.size(); t++) {
        const bool mine_t = t % mine.tile_ranks == mine.tile_rank;
        if (!mine_t && counts[t] != 0u) return RAYRS_INVALID_ARG;
        if (!mine_t) continue;
        if (counts[t] > SLOT_SAMPLE_MASK || counts[t] % c != h.samples % c) return RAYRS_INVALID_ARG;
        if ((counts[t] == 0u) != (h.samples == 0u)) return RAYRS_INVALID_ARG;  // a pass on an empty film takes every tile
        most = counts[t] > most ? counts[t] : most;
        same = same && counts[t] == h.samples;
    }
    if (most != h.samples && !counts.empty() && mine.tile_rank < counts.size()) return RAYRS_INVALID_ARG;
    RAYRS_TRY(film_enter(film));
    RAYRS_TRY(film_stage(film));
    HIP_TRY(film->d_tile_n.upload(counts.data(), film->count_bytes()));
    const uint8_t* src = static_cast<const uint8_t*>(in_host) + sizeof(h);
    uint8_t* dst = film->d_rec.as<uint8_t>();
    for (size_t at = 0, total = film->record_bytes(); at < total; at += STAGE_BYTES) {
        const size_t piece = total - at < STAGE_BYTES ? total - at : STAGE_BYTES;
        std::memcpy(film->h_stage.as<void>(), src + at, piece);
        HIP_TRY(hipMemcpyAsync(dst + at, film->h_stage.as<void>(), piece, hipMemcpyHostToDevice, nullptr));
        HIP_TRY(hipStreamSynchronize(nullptr));
    }
    film->samples = h.samples, film->rays = h.rays, film->paths = h.paths;
    film->uniform = same;
    film->closed = h.closed != 0u;
    return RAYRS_OK;
    })
}

}  // extern "C"

// ------------------------------------------------------------------ film_host.hpp: a film's view for a history

namespace rayrs {

int film_view_check(const rayrs_film* film, uint32_t feature_samples, int* device) {
    if (!film || film->samples == 0) return RAYRS_INVALID_ARG;
    if (film->prm.tile_ranks > 1u) return RAYRS_INVALID_ARG;  // reprojection reads a pixel's neighbours, as the filters do
    RAYRS_TRY(features_check(&film->camera, feature_samples, film->prm.tile_rank, film->prm.tile_ranks, film->prm.fast_traversal));
    *device = film->scene->device;
    return RAYRS_OK;
}

// (the sequence rayrs_film_denoise_guided prepares its inputs with, here with the events between its steps)
int film_view(rayrs_film* film, uint32_t feature_samples, FilmView* out, const hipEvent_t* marks) {
    RAYRS_TRY(film_enter(film));
    RAYRS_TRY(film_features(film, feature_samples));
    if (marks) HIP_TRY(hipEventRecord(marks[0], nullptr));
    const uint32_t w = film->camera.x_pixels, h = film->camera.y_pixels;
    HIP_TRY(film->d_out.reserve(frame_bytes(w, h, RAYRS_OUT_F64)));
    const CameraDev cam = make_camera_dev(&film->camera);
    HIP_TRY(launch_film_read(cam, film->share.tiles_x, film->d_rec.as<double>(), film->d_tile_n.as<uint32_t>(), RAYRS_OUT_F64,
                             film->d_out.as<>(), nullptr));
    if (marks) HIP_TRY(hipEventRecord(marks[1], nullptr));
    RAYRS_TRY(film_noise_plane(film));
    if (marks) HIP_TRY(hipEventRecord(marks[2], nullptr));
    out->scene = film->scene, out->camera = &film->camera;
    out->color = film->d_out.as<double>(), out->variance = film->d_var.as<double>();
    out->tile_n = film->d_tile_n.as<uint32_t>(), out->tiles_x = film->share.tiles_x;
    out->normal = film->feat.normal.as<double>(), out->albedo = film->feat.albedo.as<double>();
    out->depth = film->feat.depth.as<double>(), out->coverage = film->feat.coverage.as<double>();
    out->prim = film->feat.prim.as<uint32_t>();
    return RAYRS_OK;
}

}  // namespace rayrs
