// bake_abi.cpp -- the bake of include/rayrs_hip.h (BAKE: rayrs_bake_*): a bake's lifetime, a pass as launches of bake.hip's
// wave kernels (with a mesh-light group of N >= 1 triangles, MESH-LIT FILMS AND BAKES: bake_mesh.hip's) on the scene's radiance
// scratch with bake_accumulate_kernel behind each, the selection of an adaptive pass, the
// values, the counts and the noise read from the records, and the checkpoint image.  The refusals, the light table and the
// scratch's ordering rule are the light-list queries' (radiance_lit_host.hpp), piece by piece as the direct-lit films take them.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "../../include/rayrs_hip.h"
#include "bake_kernels.h"
#include "passes_mesh_kernels.h"
#include "radiance_lit_host.hpp"
#include "scene_internal.hpp"

using namespace rayrs;

namespace {
// The checkpoint image: this header, then the five record planes as they lie on the device (bake_kernels.h), then the points'
// query counts (8 bytes each), then their sample counts (4 bytes each).
constexpr uint32_t STATE_MAGIC = 0x4b414252u;  // "RBAK"
constexpr uint32_t STATE_VERSION = 1;
struct StateHeader {
    uint32_t magic, version;
    uint32_t kind, sky;
    uint32_t sample_chunk, max_bounces;
    uint32_t fast_traversal, closed;
    uint64_t seed, index_base;
    double bias;
    uint64_t n;
    uint64_t samples, rays, paths;  // samples: the largest N_i
    uint64_t record_bytes;
};
static_assert(sizeof(StateHeader) == 96, "StateHeader");
constexpr uint64_t BAKE_PASS_CHUNKS = 1ull << 16;  // a pass's chunks per point, at most
}  // namespace

struct rayrs_bake {
    rayrs_scene* scene = nullptr;  // not owned
    rayrs_bake_params prm = {};    // as given, defaults filled in
    uint64_t n = 0;
    uint64_t samples = 0, rays = 0, paths = 0;  // samples: the largest N_i
    bool closed = false;
    std::vector<uint32_t> lights;  // the list as given, fixed for the bake's life; not part of the checkpoint image
    // MESH-LIT FILMS AND BAKES: the group of rayrs_bake_create_mesh, borrowed (it outlives the bake); null or empty: none
    const rayrs_mesh_lights* mesh = nullptr;
    bool grouped() const { return mesh && mesh->n != 0u; }
    DevBuf d_a, d_b;      // the points
    DevBuf d_rec;         // bake_kernels.h: five planes of n doubles
    DevBuf d_queries;     // n x 8 bytes
    DevBuf d_count;       // N_i: n words
    DevBuf d_blocks;      // an adaptive pass: one word per workgroup of the select ...
    DevBuf d_list;        // ... and the list, one BakeRef per point at most
    DevBuf d_select;      // one BakeSelect
    PinnedBuf h_word;     // it, read back
    DevBuf d_counts;      // one BakeCounts
    DevBuf d_pass;        // one BakePassCounts, read once per pass
    DevBuf d_out;         // what rayrs_bake_read and rayrs_bake_noise copy out, grown on demand
    Event ev[2];          // around a pass's launches
    bool unlit() const { return prm.sky == 0u && lights.empty(); }
    LitCall call(uint32_t samples_) const {
        return LitCall{prm.kind == 0u ? LIT_START_POINT : LIT_START_RAY, samples_, prm.max_bounces, prm.sample_chunk, prm.bias, prm.seed,
                       prm.index_base, prm.fast_traversal, lights.data(), (uint32_t)lights.size(), true, prm.sky != 0u, mesh};
    }
    size_t record_bytes() const { return (size_t)n * BAKE_PLANES * sizeof(double); }
    size_t query_bytes() const { return (size_t)n * sizeof(unsigned long long); }
    size_t count_bytes() const { return (size_t)n * sizeof(uint32_t); }
    BakeDev dev() const { return BakeDev{d_rec.as<double>(), d_queries.as<unsigned long long>(), d_count.as<uint32_t>(), n}; }
    StateHeader header() const {
        StateHeader h;
        std::memset(&h, 0, sizeof(h));
        h.magic = STATE_MAGIC, h.version = STATE_VERSION;
        h.kind = prm.kind, h.sky = prm.sky;
        h.sample_chunk = prm.sample_chunk, h.max_bounces = prm.max_bounces;
        h.fast_traversal = prm.fast_traversal, h.closed = closed ? 1u : 0u;
        h.seed = prm.seed, h.index_base = prm.index_base, h.bias = prm.bias;
        h.n = n;
        h.samples = samples, h.rays = rays, h.paths = paths;
        h.record_bytes = record_bytes();
        return h;
    }
};

// a bake's calls run on the scene's device, behind whatever the scene still has in flight
static int bake_enter(rayrs_bake* b) { return scene_settle(b->scene); }

// One pass of n samples: over the list bake_select has just made (n_list entries, each point from the N_i the list holds), or,
// n_list == 0, over every point from its own N_i.  Whole points, as many as fit RADIANCE_LAUNCH_ITEMS items, per launch of the
// direct, the sky or (a group of N >= 1 triangles) the mesh wave on the scene's radiance scratch; behind each launch, on the same
// stream, bake_accumulate_kernel over its
// entries.  The host waits once, for the pass's query total.
static int bake_pass(rayrs_bake* bake, uint32_t n, uint32_t n_list, rayrs_bake_pass* st) {
    const auto t0 = std::chrono::steady_clock::now();
    rayrs_scene* scene = bake->scene;
    const uint32_t c = bake->prm.sample_chunk;
    const LitCall call = bake->call(n);
    const LightsDev lights = lights_resolve(scene, call);
    const LightSlotsDev slots = direct_slots(scene, call);
    const bool use_sky = bake->prm.sky != 0u;
    SkyDev sky;
    std::memset(&sky, 0, sizeof(sky));
    if (use_sky) RAYRS_TRY(sky_device_table(scene, &sky));
    MeshDev mesh;
    std::memset(&mesh, 0, sizeof(mesh));
    const bool grouped = bake->grouped();
    if (grouped) RAYRS_TRY(mesh_device_table(bake->mesh, &mesh));  // (uploaded by the handle's first call, then kept)
    const SceneDev sc = make_scene_dev(scene, bake->prm.fast_traversal == 0u);
    const hipStream_t stream = nullptr;
    RadianceDev rd;
    std::memset(&rd, 0, sizeof(rd));
    RAYRS_TRY(lit_scratch_begin(scene, sc, stream, &rd));
    rd.samples = n, rd.max_bounces = bake->prm.max_bounces, rd.irradiance = bake->prm.kind == 0u ? 1u : 0u;
    rd.chunk = c, rd.chunks = (n + c - 1u) / c;  // (n and c are below 2^30)
    rd.seed = bake->prm.seed, rd.index_base = bake->prm.index_base, rd.bias = bake->prm.bias;
    rd.a = bake->d_a.as<double>(), rd.b = bake->d_b.as<double>();  // (the whole arrays: a lane's ray is the point's index)
    const uint64_t n_entries = n_list ? n_list : bake->n;
    BakeStartDev bs;
    std::memset(&bs, 0, sizeof(bs));
    bs.list = n_list ? bake->d_list.as<BakeRef>() : nullptr;
    bs.count = bake->d_count.as<uint32_t>();
    bs.spp = n;
    const BakeDev bk = bake->dev();
    const uint32_t has_queries = rd.max_bounces != 0u ? 1u : 0u;
    BakePassCounts* counts = bake->d_pass.as<BakePassCounts>();
    HIP_TRY(hipMemsetAsync(counts, 0, sizeof(BakePassCounts), stream));
    HIP_TRY(hipEventRecord(bake->ev[0], stream));
    const uint64_t per_launch = RADIANCE_LAUNCH_ITEMS / rd.chunks;  // (>= 16: the pass-size rule)
    uint32_t launches = 0;
    for (uint64_t e0 = 0; e0 < n_entries; e0 += per_launch) {
        rd.n = (uint32_t)(n_entries - e0 < per_launch ? n_entries - e0 : per_launch);
        bs.e0 = (uint32_t)e0;
        if (!has_queries) {  // the loop runs no turn: +0 and no query, whatever the scene
            HIP_TRY(hipMemsetAsync(rd.partial, 0, (size_t)rd.n * rd.chunks * 3u * sizeof(double), stream));
        } else {
            HIP_TRY(hipMemsetAsync(rd.cursor, 0, sizeof(unsigned long long), stream));
            if (grouped) HIP_TRY(launch_bake_mesh(scene->flat.compact, sc, rd, bs, lights, slots, mesh, sky, use_sky, bake->prm.kind == 0u,
                                                  scene->cu_count, stream));
            else HIP_TRY(launch_bake_wave(scene->flat.compact, sc, rd, bs, lights, slots, use_sky ? &sky : nullptr, bake->prm.kind == 0u,
                                          scene->cu_count, stream));
            launches++;
        }
        HIP_TRY(launch_bake_accumulate(rd, bs, bk, n / c, has_queries, counts, stream));
    }
    HIP_TRY(hipEventRecord(bake->ev[1], stream));
    RAYRS_TRY(lit_scratch_end(scene, stream));
    BakePassCounts got;
    HIP_TRY(bake->d_pass.download(&got, sizeof(got)));  // (the pass's one wait)
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, bake->ev[0], bake->ev[1]));
    std::memset(st, 0, sizeof(*st));
    st->points = n_entries, st->paths = n_entries * n, st->rays = got.queries;
    st->kernel_ms = ms;
    st->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    st->launches = launches;
    bake->rays += st->rays, bake->paths += st->paths;
    return RAYRS_OK;
}

// the refusals of a pass of n samples that the bake's state decides: its length, and the sample cursor's 30 bits
static int bake_pass_unsupported(const rayrs_bake* bake, uint32_t n) {
    if (n > SLOT_SAMPLE_MASK) return RAYRS_UNSUPPORTED;
    if (((uint64_t)n + bake->prm.sample_chunk - 1u) / bake->prm.sample_chunk > BAKE_PASS_CHUNKS) return RAYRS_UNSUPPORTED;
    return RAYRS_OK;
}

static int bake_create(rayrs_scene* scene, const double* a, const double* b, uint64_t n, const rayrs_bake_params* params,
                       const uint32_t* lights, uint32_t n_lights, const rayrs_mesh_lights* mesh, rayrs_bake** out) {
    if (!scene || !a || !b || !params || !out) return RAYRS_INVALID_ARG;
    *out = nullptr;
    rayrs_bake_params prm = *params;
    if (prm.sample_chunk == 0u) prm.sample_chunk = 4u;
    if (prm.fast_traversal > 1u || prm.kind > 1u || prm.sky > 1u || prm.pad != 0u) return RAYRS_INVALID_ARG;
    const LitCall list{prm.kind == 0u ? LIT_START_POINT : LIT_START_RAY, prm.sample_chunk, prm.max_bounces, prm.sample_chunk, prm.bias,
                       prm.seed, prm.index_base, prm.fast_traversal, lights, n_lights, true, prm.sky != 0u};
    RAYRS_TRY(lit_list_invalid(scene, list));
    if (mesh && mesh->scene != scene) return RAYRS_INVALID_ARG;
    if (mesh && mesh->tree) return RAYRS_UNSUPPORTED;  // LIGHT TREE: the passes have no kernel that descends a tree
    if (prm.sample_chunk > SLOT_SAMPLE_MASK || prm.max_bounces > 8000u) return RAYRS_UNSUPPORTED;
    // (an item is one chunk of at most max_bounces, with shadow rays 2 * max_bounces + 1, queries a sample, counted in 32 bits)
    const bool unlit = prm.sky == 0u && n_lights == 0u && !(mesh && mesh->n != 0u);  // (a group's paths have shadow rays)
    const uint64_t path_queries = unlit ? (uint64_t)prm.max_bounces : 2ull * prm.max_bounces + 1u;
    if ((uint64_t)prm.sample_chunk * path_queries >= (1ull << 32)) return RAYRS_UNSUPPORTED;
    RAYRS_TRY(lit_list_unsupported(scene, list));
    if (n >= (1ull << 32)) return RAYRS_UNSUPPORTED;
    if (scene->device < 0) return RAYRS_NO_DEVICE;
    std::unique_ptr<rayrs_bake> k(new rayrs_bake());
    k->scene = scene;
    k->prm = prm;
    k->n = n;
    k->lights.assign(lights, lights + n_lights);
    k->mesh = mesh;
    HIP_TRY(hipSetDevice(scene->device));
    if (n) {
        HIP_TRY(k->d_a.upload(a, (size_t)n * 3u * sizeof(double)));
        HIP_TRY(k->d_b.upload(b, (size_t)n * 3u * sizeof(double)));
        HIP_TRY(k->d_rec.reserve(k->record_bytes()));
        HIP_TRY(hipMemset(k->d_rec.as<>(), 0, k->record_bytes()));
        HIP_TRY(k->d_queries.reserve(k->query_bytes()));
        HIP_TRY(hipMemset(k->d_queries.as<>(), 0, k->query_bytes()));
        HIP_TRY(k->d_count.reserve(k->count_bytes()));
        HIP_TRY(hipMemset(k->d_count.as<>(), 0, k->count_bytes()));
    }
    HIP_TRY(k->d_select.reserve(sizeof(BakeSelect)));
    HIP_TRY(k->h_word.alloc(sizeof(BakeSelect)));
    HIP_TRY(k->d_counts.reserve(sizeof(BakeCounts)));
    HIP_TRY(k->d_pass.reserve(sizeof(BakePassCounts)));
    HIP_TRY(k->ev[0].create());
    HIP_TRY(k->ev[1].create());
    *out = k.release();
    return RAYRS_OK;
}

extern "C" {

int rayrs_bake_create(rayrs_scene* scene, const double* a, const double* b, uint64_t n, const rayrs_bake_params* params,
                      const uint32_t* lights, uint32_t n_lights, rayrs_bake** out) {
    RAYRS_GUARDED({ return bake_create(scene, a, b, n, params, lights, n_lights, nullptr, out); })
}

int rayrs_bake_create_mesh(rayrs_scene* scene, const double* a, const double* b, uint64_t n, const rayrs_bake_params* params,
                           const uint32_t* lights, uint32_t n_lights, const rayrs_mesh_lights* mesh, rayrs_bake** out) {
    RAYRS_GUARDED({ return bake_create(scene, a, b, n, params, lights, n_lights, mesh, out); })
}

void rayrs_bake_destroy(rayrs_bake* bake) {
    if (!bake) return;
    // (the scene outlives its bakes: the header's rule)
    if (bake->scene && bake->scene->device >= 0) (void)hipSetDevice(bake->scene->device);
    delete bake;
}

int rayrs_bake_render(rayrs_bake* bake, uint32_t n, rayrs_bake_pass* stats) {
    RAYRS_GUARDED({
    if (!bake || n == 0u || bake->closed) return RAYRS_INVALID_ARG;
    RAYRS_TRY(bake_pass_unsupported(bake, n));
    if (bake->samples > SLOT_SAMPLE_MASK || n > SLOT_SAMPLE_MASK - (uint32_t)bake->samples) return RAYRS_UNSUPPORTED;
    RAYRS_TRY(bake_enter(bake));
    rayrs_bake_pass st;
    std::memset(&st, 0, sizeof(st));
    if (bake->n) {
        RAYRS_TRY(bake_pass(bake, n, 0u, &st));
        bake->samples += n;
    }
    if (n % bake->prm.sample_chunk != 0u) bake->closed = true;
    if (stats) *stats = st;
    return RAYRS_OK;
    })
}

int rayrs_bake_render_adaptive(rayrs_bake* bake, uint32_t n, double tau, uint32_t max_point_samples, uint64_t* active_points,
                               rayrs_bake_pass* stats) {
    RAYRS_GUARDED({
    if (!bake || n == 0u || bake->closed || !(tau >= 0.0) || !std::isfinite(tau)) return RAYRS_INVALID_ARG;
    if (n % bake->prm.sample_chunk != 0u) return RAYRS_INVALID_ARG;
    RAYRS_TRY(bake_pass_unsupported(bake, n));
    RAYRS_TRY(bake_enter(bake));
    const uint32_t cap = max_point_samples != 0u && max_point_samples < SLOT_SAMPLE_MASK ? max_point_samples : SLOT_SAMPLE_MASK;
    rayrs_bake_pass st;
    std::memset(&st, 0, sizeof(st));
    BakeSelect got = {0u, 0u};
    if (bake->n) {
        // the list of the pass; one 8-byte word of the result comes back through the bake's pinned word -- the list's length,
        // which the pass is planned from, and the largest count it leaves -- and that copy is the only wait
        HIP_TRY(bake->d_blocks.reserve((size_t)bake_select_blocks(bake->n) * sizeof(uint32_t)));
        HIP_TRY(bake->d_list.reserve((size_t)bake->n * sizeof(BakeRef)));
        BakeSelect* sel = bake->d_select.as<BakeSelect>();
        HIP_TRY(launch_bake_select(bake->dev(), bake->prm.sample_chunk, n, cap, tau * tau, bake->d_blocks.as<uint32_t>(),
                                   bake->d_list.as<BakeRef>(), sel, nullptr));
        BakeSelect* h_word = bake->h_word.as<BakeSelect>();
        HIP_TRY(hipMemcpyAsync(h_word, sel, sizeof(BakeSelect), hipMemcpyDeviceToHost, nullptr));
        HIP_TRY(hipStreamSynchronize(nullptr));
        got = *h_word;
    }
    if (got.n_active != 0u) {
        RAYRS_TRY(bake_pass(bake, n, got.n_active, &st));
        if (got.max_after > bake->samples) bake->samples = got.max_after;
    }
    if (active_points) *active_points = got.n_active;
    if (stats) *stats = st;
    return RAYRS_OK;
    })
}

int rayrs_bake_read(rayrs_bake* bake, double* radiance, uint64_t* queries) {
    RAYRS_GUARDED({
    if (!bake || (!radiance && !queries)) return RAYRS_INVALID_ARG;
    if (bake->n == 0u) return RAYRS_OK;
    RAYRS_TRY(bake_enter(bake));
    if (radiance) {
        const size_t bytes = (size_t)bake->n * 3u * sizeof(double);
        HIP_TRY(bake->d_out.reserve(bytes));
        HIP_TRY(launch_bake_read(bake->dev(), bake->d_out.as<double>(), nullptr));
        HIP_TRY(bake->d_out.download(radiance, bytes));
    }
    if (queries) HIP_TRY(bake->d_queries.download(queries, bake->query_bytes()));
    return RAYRS_OK;
    })
}

int rayrs_bake_point_samples(rayrs_bake* bake, uint32_t* out) {
    RAYRS_GUARDED({
    if (!bake || !out) return RAYRS_INVALID_ARG;
    if (bake->n == 0u) return RAYRS_OK;
    RAYRS_TRY(bake_enter(bake));
    HIP_TRY(bake->d_count.download(out, bake->count_bytes()));
    return RAYRS_OK;
    })
}

int rayrs_bake_noise(rayrs_bake* bake, double* variance) {
    RAYRS_GUARDED({
    if (!bake || !variance) return RAYRS_INVALID_ARG;
    if (bake->n == 0u) return RAYRS_OK;
    RAYRS_TRY(bake_enter(bake));
    const size_t bytes = (size_t)bake->n * sizeof(double);
    HIP_TRY(bake->d_out.reserve(bytes));
    HIP_TRY(launch_bake_noise(bake->dev(), bake->prm.sample_chunk, bake->d_out.as<double>(), nullptr));
    HIP_TRY(bake->d_out.download(variance, bytes));
    return RAYRS_OK;
    })
}

int rayrs_bake_status_get(rayrs_bake* bake, double tau, rayrs_bake_status* out) {
    RAYRS_GUARDED({
    if (!bake || !out || !(tau >= 0.0) || !std::isfinite(tau)) return RAYRS_INVALID_ARG;
    RAYRS_TRY(bake_enter(bake));
    BakeCounts c;
    std::memset(&c, 0, sizeof(c));
    if (bake->n) {
        HIP_TRY(hipMemsetAsync(bake->d_counts.as<>(), 0, sizeof(BakeCounts), nullptr));
        HIP_TRY(launch_bake_status(bake->dev(), bake->prm.sample_chunk, tau * tau, bake->d_counts.as<BakeCounts>(), nullptr));
        HIP_TRY(bake->d_counts.download(&c, sizeof(c)));
        bake->samples = c.max_samples;  // (what the passes have kept it at)
    }
    std::memset(out, 0, sizeof(*out));
    out->samples = bake->samples, out->rays = bake->rays, out->paths = bake->paths;
    out->unconverged = c.unconverged, out->nonfinite = c.nonfinite;
    out->points = bake->n;
    out->closed = bake->closed ? 1u : 0u;
    return RAYRS_OK;
    })
}

uint64_t rayrs_bake_state_bytes(const rayrs_bake* bake) {
    return bake ? sizeof(StateHeader) + bake->record_bytes() + bake->query_bytes() + bake->count_bytes() : 0;
}

int rayrs_bake_state_get(rayrs_bake* bake, void* out_host, uint64_t cap) {
    RAYRS_GUARDED({
    if (!bake || !out_host || cap < rayrs_bake_state_bytes(bake)) return RAYRS_INVALID_ARG;
    RAYRS_TRY(bake_enter(bake));
    const StateHeader h = bake->header();
    uint8_t* dst = static_cast<uint8_t*>(out_host);
    std::memcpy(dst, &h, sizeof(h));
    dst += sizeof(h);
    HIP_TRY(bake->d_rec.download(dst, bake->record_bytes()));
    dst += bake->record_bytes();
    HIP_TRY(bake->d_queries.download(dst, bake->query_bytes()));
    dst += bake->query_bytes();
    HIP_TRY(bake->d_count.download(dst, bake->count_bytes()));
    return RAYRS_OK;
    })
}

int rayrs_bake_state_set(rayrs_bake* bake, const void* in_host, uint64_t bytes) {
    RAYRS_GUARDED({
    if (!bake || !in_host || bytes < sizeof(StateHeader)) return RAYRS_INVALID_ARG;
    StateHeader h;
    std::memcpy(&h, in_host, sizeof(h));
    const StateHeader mine = bake->header();
    if (h.magic != STATE_MAGIC || h.version != STATE_VERSION) return RAYRS_INVALID_ARG;
    if (h.kind != mine.kind || h.sky != mine.sky || h.sample_chunk != mine.sample_chunk || h.max_bounces != mine.max_bounces ||
        h.fast_traversal != mine.fast_traversal || h.seed != mine.seed || h.index_base != mine.index_base ||
        std::memcmp(&h.bias, &mine.bias, sizeof(double)) != 0 || h.n != mine.n)
        return RAYRS_INVALID_ARG;
    if (h.record_bytes != mine.record_bytes || bytes != rayrs_bake_state_bytes(bake)) return RAYRS_INVALID_ARG;
    // counters that no sequence of passes leaves behind: not this library's image
    const uint64_t c = mine.sample_chunk;
    if (h.closed > 1u || h.samples > SLOT_SAMPLE_MASK || (h.closed == 0u && h.samples % c != 0u) || (h.closed != 0u && h.n != 0u && h.samples % c == 0u))
        return RAYRS_INVALID_ARG;
    // ... and per-point counts that none leaves: in an open bake whole chunks, in a closed one the same short chunk
    // everywhere; the largest is the header's
    const uint8_t* src = static_cast<const uint8_t*>(in_host) + sizeof(h);
    std::vector<uint32_t> counts((size_t)bake->n);
    if (bake->n) std::memcpy(counts.data(), src + bake->record_bytes() + bake->query_bytes(), bake->count_bytes());
    uint32_t most = 0;
    for (size_t i = 0; i < counts.size(); i++) {
        if (counts[i] > SLOT_SAMPLE_MASK || counts[i] % c != h.samples % c) return RAYRS_INVALID_ARG;
        most = counts[i] > most ? counts[i] : most;
    }
    if (most != h.samples) return RAYRS_INVALID_ARG;
    RAYRS_TRY(bake_enter(bake));
    if (bake->n) {
        HIP_TRY(hipMemcpy(bake->d_rec.as<>(), src, bake->record_bytes(), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(bake->d_queries.as<>(), src + bake->record_bytes(), bake->query_bytes(), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(bake->d_count.as<>(), counts.data(), bake->count_bytes(), hipMemcpyHostToDevice));
    }
    bake->samples = h.samples, bake->rays = h.rays, bake->paths = h.paths;
    bake->closed = h.closed != 0u;
    return RAYRS_OK;
    })
}

}  // extern "C"
