// radiance_abi.cpp -- radiance queries of include/rayrs_hip.h (RADIANCE QUERY, IRRADIANCE): the refusals, a batch of rays or
// points through launches of radiance.hip's kernels on the caller's stream, the host forms around them (upload, launch, wait,
// download), and the lab's hooks (rayrs_lab.h rayrs_lab_radiance_tuning, rayrs_lab_radiance_turns).
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/rayrs_hip.h"
#include "radiance_kernels.h"
#include "scene_internal.hpp"

using namespace rayrs;

namespace {

// What a call asks for, beside its buffers.
struct RadianceCall {
    uint32_t irradiance;
    uint32_t samples, max_bounces, sample_chunk;
    double bias;
    uint64_t seed, index_base;
    uint32_t fast_traversal;
};

// The refusals that need no device, in the header's order.
int radiance_check(const rayrs_scene* scene, const void* a, const void* b, const void* radiance, const void* queries,
                   const RadianceCall& c) {
    if (!scene || !a || !b || (!radiance && !queries)) return RAYRS_INVALID_ARG;
    if (c.samples == 0u || c.fast_traversal > 1u) return RAYRS_INVALID_ARG;
    if (c.samples > SLOT_SAMPLE_MASK || c.max_bounces > 8000u) return RAYRS_UNSUPPORTED;  // rayrs_render_params' limits
    if ((uint64_t)c.samples * c.max_bounces >= (1ull << 32)) return RAYRS_UNSUPPORTED;   // queries_i could wrap
    if (radiance_chunks(c.samples, c.sample_chunk) > RADIANCE_LAUNCH_ITEMS) return RAYRS_UNSUPPORTED;  // a launch takes whole rays
    if (scene->device < 0) return RAYRS_NO_DEVICE;
    return RAYRS_OK;
}

// The batch, whole rays of at most RADIANCE_LAUNCH_ITEMS items per launch, all on `stream`: a, b and the outputs are the whole
// batch's, and move on from launch to launch with index_base.  The launches share the scene's scratch and the queries' stack
// strip, under the strip's ordering rule (scene_internal.hpp rayrs_scene::Queries): a user on another stream waits on the
// device for the last one.  The scratch is reserved at a launch's largest size, so only a scene's first call allocates.
int radiance_enqueue(rayrs_scene* scene, const RadianceCall& c, const double* a, const double* b, uint64_t n, double* radiance,
                     uint32_t* queries, unsigned long long* turns, hipStream_t stream) {
    if (c.max_bounces == 0u) {  // the loop runs no turn: +0 and no query, whatever the scene
        if (radiance) HIP_TRY(hipMemsetAsync(radiance, 0, n * 3u * sizeof(double), stream));
        if (queries) HIP_TRY(hipMemsetAsync(queries, 0, n * sizeof(uint32_t), stream));
        return RAYRS_OK;
    }
    const SceneDev sc = make_scene_dev(scene, c.fast_traversal == 0u);
    rayrs_scene::Queries& strip = scene->queries;
    rayrs_scene::Radiance& own = scene->radiance;
    if (sc.stack_depth > sc.stack_lds) HIP_TRY(strip.d_stack_spill.reserve(stack_spill_words(sc, QUERY_LAUNCH_RAYS) * sizeof(uint32_t)));
    HIP_TRY(own.d_scratch.reserve(RADIANCE_SCRATCH_BYTES));
    if (!strip.has_event) {
        HIP_TRY(strip.ev_done.create());
        strip.has_event = true;
    }
    if (strip.strip_in_use) HIP_TRY(hipStreamWaitEvent(stream, strip.ev_done, 0));

    RadianceDev rd;
    std::memset(&rd, 0, sizeof(rd));
    rd.samples = c.samples, rd.max_bounces = c.max_bounces, rd.irradiance = c.irradiance;
    rd.chunk = radiance_chunk(c.samples, c.sample_chunk), rd.chunks = radiance_chunks(c.samples, c.sample_chunk);
    rd.refill_below = own.refill_below ? own.refill_below : RADIANCE_REFILL_BELOW;
    rd.shade_at = own.shade_at ? own.shade_at : RADIANCE_SHADE_AT;
    rd.leaf_min = own.leaf_min ? own.leaf_min : RADIANCE_LEAF_MIN;
    rd.seed = c.seed, rd.bias = c.bias;
    char* scratch = own.d_scratch.as<char>();
    rd.cursor = reinterpret_cast<unsigned long long*>(scratch);
    rd.partial = reinterpret_cast<double*>(scratch + RADIANCE_CURSOR_BYTES);
    rd.partial_queries = reinterpret_cast<uint32_t*>(scratch + RADIANCE_CURSOR_BYTES + RADIANCE_LAUNCH_ITEMS * 24u);
    rd.turns = turns;
    rd.spill = strip.d_stack_spill.as<uint32_t>();
    const uint64_t per_launch = RADIANCE_LAUNCH_ITEMS / rd.chunks;  // (>= 1: radiance_check)
    for (uint64_t base = 0; base < n; base += per_launch) {
        rd.n = (uint32_t)(n - base < per_launch ? n - base : per_launch);
        rd.index_base = c.index_base + base;
        rd.a = a + base * 3u, rd.b = b + base * 3u;
        rd.radiance = radiance ? radiance + base * 3u : nullptr;
        rd.queries = queries ? queries + base : nullptr;
        HIP_TRY(hipMemsetAsync(rd.cursor, 0, sizeof(unsigned long long), stream));
        HIP_TRY(launch_radiance(scene->flat.compact, sc, rd, scene->cu_count, stream));
    }
    HIP_TRY(hipEventRecord(strip.ev_done, stream));
    strip.strip_in_use = true;
    return RAYRS_OK;
}

// The host form -- upload, launch on the null stream, wait, download -- and the lab's with `turns`.
int radiance_host(rayrs_scene* scene, const RadianceCall& c, const double* a, const double* b, uint64_t n, double* radiance,
                  uint32_t* queries, unsigned long long* turns) {
    HIP_TRY(hipSetDevice(scene->device));
    rayrs_scene::Radiance& own = scene->radiance;
    HIP_TRY(own.d_a.upload(a, n * 3u * sizeof(double)));
    HIP_TRY(own.d_b.upload(b, n * 3u * sizeof(double)));
    if (radiance) HIP_TRY(own.d_radiance.reserve(n * 3u * sizeof(double)));
    if (queries) HIP_TRY(own.d_queries.reserve(n * sizeof(uint32_t)));
    unsigned long long* d_turns = nullptr;
    if (turns) {
        HIP_TRY(own.d_turns.reserve(3u * sizeof(unsigned long long)));
        HIP_TRY(hipMemsetAsync(own.d_turns.as<>(), 0, 3u * sizeof(unsigned long long), nullptr));
        d_turns = own.d_turns.as<unsigned long long>();
    }
    RAYRS_TRY(radiance_enqueue(scene, c, own.d_a.as<double>(), own.d_b.as<double>(), n, radiance ? own.d_radiance.as<double>() : nullptr,
                               queries ? own.d_queries.as<uint32_t>() : nullptr, d_turns, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    if (radiance) HIP_TRY(own.d_radiance.download(radiance, n * 3u * sizeof(double)));
    if (queries) HIP_TRY(own.d_queries.download(queries, n * sizeof(uint32_t)));
    if (turns) HIP_TRY(own.d_turns.download(turns, 3u * sizeof(unsigned long long)));
    return RAYRS_OK;
}

int radiance_entry(rayrs_scene* scene, const RadianceCall& c, const double* a, const double* b, uint64_t n, double* radiance,
                   uint32_t* queries, bool launch, void* hip_stream) {
    RAYRS_TRY(radiance_check(scene, a, b, radiance, queries, c));
    if (n == 0u) return RAYRS_OK;
    if (!launch) return radiance_host(scene, c, a, b, n, radiance, queries, nullptr);
    HIP_TRY(hipSetDevice(scene->device));
    return radiance_enqueue(scene, c, a, b, n, radiance, queries, nullptr, reinterpret_cast<hipStream_t>(hip_stream));
}

}  // namespace

extern "C" {

int rayrs_scene_radiance(rayrs_scene* scene, const double* origin, const double* direction, uint64_t n, uint32_t samples,
                         uint32_t max_bounces, uint32_t sample_chunk, uint64_t seed, uint64_t index_base, uint32_t fast_traversal,
                         double* radiance, uint32_t* queries) {
    RAYRS_GUARDED({
    return radiance_entry(scene, RadianceCall{0u, samples, max_bounces, sample_chunk, 0.0, seed, index_base, fast_traversal}, origin,
                          direction, n, radiance, queries, false, nullptr);
    })
}

int rayrs_scene_radiance_launch(rayrs_scene* scene, const double* origin, const double* direction, uint64_t n, uint32_t samples,
                                uint32_t max_bounces, uint32_t sample_chunk, uint64_t seed, uint64_t index_base,
                                uint32_t fast_traversal, double* radiance, uint32_t* queries, void* hip_stream) {
    RAYRS_GUARDED({
    return radiance_entry(scene, RadianceCall{0u, samples, max_bounces, sample_chunk, 0.0, seed, index_base, fast_traversal}, origin,
                          direction, n, radiance, queries, true, hip_stream);
    })
}

int rayrs_scene_irradiance(rayrs_scene* scene, const double* position, const double* normal, uint64_t n, uint32_t samples,
                           uint32_t max_bounces, uint32_t sample_chunk, double bias, uint64_t seed, uint64_t index_base,
                           uint32_t fast_traversal, double* radiance, uint32_t* queries) {
    RAYRS_GUARDED({
    return radiance_entry(scene, RadianceCall{1u, samples, max_bounces, sample_chunk, bias, seed, index_base, fast_traversal}, position,
                          normal, n, radiance, queries, false, nullptr);
    })
}

int rayrs_scene_irradiance_launch(rayrs_scene* scene, const double* position, const double* normal, uint64_t n, uint32_t samples,
                                  uint32_t max_bounces, uint32_t sample_chunk, double bias, uint64_t seed, uint64_t index_base,
                                  uint32_t fast_traversal, double* radiance, uint32_t* queries, void* hip_stream) {
    RAYRS_GUARDED({
    return radiance_entry(scene, RadianceCall{1u, samples, max_bounces, sample_chunk, bias, seed, index_base, fast_traversal}, position,
                          normal, n, radiance, queries, true, hip_stream);
    })
}

int rayrs_lab_radiance_tuning(rayrs_scene* scene, uint32_t refill_below, uint32_t shade_at, uint32_t leaf_min) {
    if (!scene || refill_below > 64u || shade_at > 64u || leaf_min > 64u) return RAYRS_INVALID_ARG;
    scene->radiance.refill_below = refill_below, scene->radiance.shade_at = shade_at, scene->radiance.leaf_min = leaf_min;
    return RAYRS_OK;
}

int rayrs_lab_radiance_turns(rayrs_scene* scene, uint32_t irradiance, const double* a, const double* b, uint64_t n, uint32_t samples,
                             uint32_t max_bounces, uint32_t sample_chunk, double bias, uint64_t seed, uint64_t index_base,
                             uint32_t fast_traversal, uint32_t* queries, uint64_t turns[3]) {
    RAYRS_GUARDED({
    const RadianceCall c{irradiance ? 1u : 0u, samples, max_bounces, sample_chunk, bias, seed, index_base, fast_traversal};
    RAYRS_TRY(radiance_check(scene, a, b, queries, turns, c));
    if (!queries || !turns) return RAYRS_INVALID_ARG;
    turns[0] = turns[1] = turns[2] = 0u;
    if (n == 0u || max_bounces == 0u) return RAYRS_OK;
    unsigned long long got[3] = {0ull, 0ull, 0ull};
    RAYRS_TRY(radiance_host(scene, c, a, b, n, nullptr, queries, got));
    turns[0] = got[0], turns[1] = got[1], turns[2] = got[2];
    return RAYRS_OK;
    })
}

}  // extern "C"
