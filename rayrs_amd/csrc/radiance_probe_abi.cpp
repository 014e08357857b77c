// radiance_probe_abi.cpp -- SH probes of include/rayrs_hip.h (SH PROBES): the refusals, a batch of probes through launches of
// radiance_probe.hip's kernels on the caller's stream (the wave of the call's lighting, then the projection in rounds), the host
// form around them, the two host-only calls over radiance_probe_table.h's functions, and the lab's hook (rayrs_lab.h
// rayrs_lab_probe_project_ms).  The list's refusals, the light table,
// the slots, the groups' and the sky's device copies and the scratch's ordering rule are the lit queries' (radiance_lit_host.hpp).
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/rayrs_hip.h"
#include "radiance_lit_host.hpp"
#include "radiance_probe_kernels.h"
#include "radiance_probe_table.h"
#include "rayrs_lab.h"
#include "scene_internal.hpp"

using namespace rayrs;

namespace {

// The refusals that need no device, in the header's order.
int probe_check(rayrs_scene* scene, const void* position, const void* coeffs, const LitCall& c, uint32_t sky) {
    if (!scene || !position || !coeffs) return RAYRS_INVALID_ARG;
    if (c.samples == 0u || c.fast_traversal > 1u || sky > 1u) return RAYRS_INVALID_ARG;
    RAYRS_TRY(lit_list_invalid(scene, c));
    if (c.mesh && c.mesh->scene != scene) return RAYRS_INVALID_ARG;
    if (c.samples > PROBE_MAX_SAMPLES || c.max_bounces > 8000u) return RAYRS_UNSUPPORTED;
    if ((uint64_t)c.samples * (2ull * c.max_bounces + 1u) >= (1ull << 32)) return RAYRS_UNSUPPORTED;
    RAYRS_TRY(lit_list_unsupported(scene, c));
    if (scene->device < 0) return RAYRS_NO_DEVICE;
    return RAYRS_OK;
}

// The projection of a launch's pd.n probes, in rounds of at most PROBE_CHUNK_SLOTS (probe, chunk) pairs.
int probe_project_rounds(ProbeDev pd, hipStream_t stream) {
    const uint32_t all_pairs = pd.n * pd.chunks;  // (<= n * S <= 2^20)
    for (uint32_t pair0 = 0; pair0 < all_pairs; pair0 += PROBE_CHUNK_SLOTS) {
        pd.pair0 = pair0;
        pd.pairs = all_pairs - pair0 < PROBE_CHUNK_SLOTS ? all_pairs - pair0 : PROBE_CHUNK_SLOTS;
        HIP_TRY(launch_probe_project(pd, stream));
    }
    return RAYRS_OK;
}

// The projection's buffer, allocated at the scene's first probe call, as the kernels take it.
int probe_chunk_buffer(rayrs_scene* scene, ProbeDev* pd) {
    HIP_TRY(scene->probes.d_chunks.reserve(PROBE_CHUNK_BYTES));
    pd->slots = scene->probes.d_chunks.as<double>();
    pd->slot_queries = reinterpret_cast<uint32_t*>(pd->slots + (size_t)PROBE_PLANES * PROBE_CHUNK_SLOTS);
    return RAYRS_OK;
}

// The batch, whole probes of at most RADIANCE_LAUNCH_ITEMS samples per launch, all on `stream`, on the radiance queries'
// scratch and strip under their ordering rule; the projection's buffer is used between the same two events.
int probe_enqueue(rayrs_scene* scene, const LitCall& c, const SceneDev& sc, const double* position, uint64_t n, double* coeffs,
                  uint32_t* queries, hipStream_t stream) {
    SkyDev sky;
    std::memset(&sky, 0, sizeof(sky));
    if (c.sky) RAYRS_TRY(sky_device_table(scene, &sky));
    const bool grouped = c.mesh && c.mesh->n != 0u;
    const bool treed = grouped && c.mesh->tree;
    MeshDev mesh;
    std::memset(&mesh, 0, sizeof(mesh));
    TreeDev tree;
    std::memset(&tree, 0, sizeof(tree));
    if (treed) RAYRS_TRY(tree_device_table(c.mesh, &tree));
    else if (grouped) RAYRS_TRY(mesh_device_table(c.mesh, &mesh));
    if (c.max_bounces == 0u) {  // the loop runs no turn: every L_s is +0 and no query is made
        HIP_TRY(hipMemsetAsync(coeffs, 0, n * PROBE_PLANES * sizeof(double), stream));
        if (queries) HIP_TRY(hipMemsetAsync(queries, 0, n * sizeof(uint32_t), stream));
        return RAYRS_OK;
    }
    const LightsDev lights = lights_resolve(scene, c);
    const LightSlotsDev slots = direct_slots(scene, c);
    RadianceDev rd;
    std::memset(&rd, 0, sizeof(rd));
    RAYRS_TRY(lit_scratch_begin(scene, sc, stream, &rd));
    rd.samples = c.samples, rd.max_bounces = c.max_bounces;
    rd.chunk = 1u, rd.chunks = c.samples;  // the wave's items: one sample each
    rd.seed = c.seed;
    ProbeDev pd;
    std::memset(&pd, 0, sizeof(pd));
    pd.samples = c.samples, pd.seed = c.seed;
    pd.chunk = radiance_chunk(c.samples, c.sample_chunk), pd.chunks = radiance_chunks(c.samples, c.sample_chunk);
    pd.partial = rd.partial, pd.partial_queries = rd.partial_queries;
    RAYRS_TRY(probe_chunk_buffer(scene, &pd));
    const uint64_t per_launch = RADIANCE_LAUNCH_ITEMS / c.samples;  // (>= 1: probe_check)
    for (uint64_t base = 0; base < n; base += per_launch) {
        rd.n = (uint32_t)(n - base < per_launch ? n - base : per_launch);
        rd.index_base = c.index_base + base;
        rd.a = position + base * 3u;
        HIP_TRY(hipMemsetAsync(rd.cursor, 0, sizeof(unsigned long long), stream));
        HIP_TRY(launch_probe_wave(scene->flat.compact, sc, rd, lights, slots, grouped && !treed ? &mesh : nullptr, treed ? &tree : nullptr, sky,
                                  c.sky, scene->cu_count, stream));
        pd.n = rd.n, pd.index_base = rd.index_base;
        pd.coeffs = coeffs + base * PROBE_PLANES;
        pd.queries = queries ? queries + base : nullptr;
        RAYRS_TRY(probe_project_rounds(pd, stream));
    }
    return lit_scratch_end(scene, stream);
}

int probe_host(rayrs_scene* scene, const LitCall& c, const SceneDev& sc, const double* position, uint64_t n, double* coeffs,
               uint32_t* queries) {
    rayrs_scene::Radiance& own = scene->radiance;
    HIP_TRY(own.d_a.upload(position, n * 3u * sizeof(double)));
    HIP_TRY(own.d_radiance.reserve(n * PROBE_PLANES * sizeof(double)));
    if (queries) HIP_TRY(own.d_queries.reserve(n * sizeof(uint32_t)));
    RAYRS_TRY(probe_enqueue(scene, c, sc, own.d_a.as<double>(), n, own.d_radiance.as<double>(),
                            queries ? own.d_queries.as<uint32_t>() : nullptr, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(own.d_radiance.download(coeffs, n * PROBE_PLANES * sizeof(double)));
    if (queries) HIP_TRY(own.d_queries.download(queries, n * sizeof(uint32_t)));
    return RAYRS_OK;
}

int probe_entry(rayrs_scene* scene, const double* position, uint64_t n, uint32_t samples, uint32_t max_bounces, uint32_t sample_chunk,
                uint64_t seed, uint64_t index_base, uint32_t fast_traversal, const uint32_t* lights, uint32_t n_lights,
                const rayrs_mesh_lights* mesh, uint32_t sky, double* coeffs, uint32_t* queries, bool launch, void* hip_stream) {
    const LitCall c{LIT_START_PROBE, samples, max_bounces, sample_chunk, 0.0, seed, index_base, fast_traversal, lights, n_lights, true,
                    sky == 1u, mesh};
    RAYRS_TRY(probe_check(scene, position, coeffs, c, sky));
    if (n == 0u) return RAYRS_OK;
    HIP_TRY(hipSetDevice(scene->device));
    const SceneDev sc = make_scene_dev(scene, fast_traversal == 0u);
    if (!launch) return probe_host(scene, c, sc, position, n, coeffs, queries);
    return probe_enqueue(scene, c, sc, position, n, coeffs, queries, reinterpret_cast<hipStream_t>(hip_stream));
}

}  // namespace

extern "C" {

int rayrs_scene_probes(rayrs_scene* scene, const double* position, uint64_t n, uint32_t samples, uint32_t max_bounces,
                       uint32_t sample_chunk, uint64_t seed, uint64_t index_base, uint32_t fast_traversal, const uint32_t* lights,
                       uint32_t n_lights, const rayrs_mesh_lights* mesh, uint32_t sky, double* coeffs, uint32_t* queries) {
    RAYRS_GUARDED({
    return probe_entry(scene, position, n, samples, max_bounces, sample_chunk, seed, index_base, fast_traversal, lights, n_lights, mesh, sky,
                       coeffs, queries, false, nullptr);
    })
}

int rayrs_scene_probes_launch(rayrs_scene* scene, const double* position, uint64_t n, uint32_t samples, uint32_t max_bounces,
                              uint32_t sample_chunk, uint64_t seed, uint64_t index_base, uint32_t fast_traversal, const uint32_t* lights,
                              uint32_t n_lights, const rayrs_mesh_lights* mesh, uint32_t sky, double* coeffs, uint32_t* queries,
                              void* hip_stream) {
    RAYRS_GUARDED({
    return probe_entry(scene, position, n, samples, max_bounces, sample_chunk, seed, index_base, fast_traversal, lights, n_lights, mesh, sky,
                       coeffs, queries, true, hip_stream);
    })
}

int rayrs_lab_probe_project_ms(rayrs_scene* scene, uint32_t n, uint32_t samples, uint32_t sample_chunk, uint32_t repeats, float* ms) {
    RAYRS_GUARDED({
    if (!scene || !ms || n == 0u || samples == 0u || repeats == 0u) return RAYRS_INVALID_ARG;
    if (samples > PROBE_MAX_SAMPLES || (uint64_t)n * samples > RADIANCE_LAUNCH_ITEMS) return RAYRS_UNSUPPORTED;
    if (scene->device < 0) return RAYRS_NO_DEVICE;
    RAYRS_TRY(scene_settle(scene));
    HIP_TRY(hipDeviceSynchronize());  // (the queries' launches are not a frame: nothing else is waited for them here)
    rayrs_scene::Radiance& own = scene->radiance;
    HIP_TRY(own.d_scratch.reserve(RADIANCE_SCRATCH_BYTES));
    HIP_TRY(own.d_radiance.reserve((size_t)n * PROBE_PLANES * sizeof(double)));
    HIP_TRY(own.d_queries.reserve((size_t)n * sizeof(uint32_t)));
    ProbeDev pd;
    std::memset(&pd, 0, sizeof(pd));
    pd.n = n, pd.samples = samples, pd.seed = 0x5EEDu, pd.index_base = 0u;
    pd.chunk = radiance_chunk(samples, sample_chunk), pd.chunks = radiance_chunks(samples, sample_chunk);
    char* scratch = own.d_scratch.as<char>();
    pd.partial = reinterpret_cast<const double*>(scratch + RADIANCE_CURSOR_BYTES);
    pd.partial_queries = reinterpret_cast<const uint32_t*>(scratch + RADIANCE_CURSOR_BYTES + RADIANCE_LAUNCH_ITEMS * 24u);
    RAYRS_TRY(probe_chunk_buffer(scene, &pd));
    pd.coeffs = own.d_radiance.as<double>(), pd.queries = own.d_queries.as<uint32_t>();
    Event start, end;
    HIP_TRY(start.create());
    HIP_TRY(end.create());
    RAYRS_TRY(probe_project_rounds(pd, nullptr));  // (a warm-up)
    HIP_TRY(hipEventRecord(start, nullptr));
    for (uint32_t r = 0; r < repeats; r++) RAYRS_TRY(probe_project_rounds(pd, nullptr));
    HIP_TRY(hipEventRecord(end, nullptr));
    HIP_TRY(hipEventSynchronize(end));
    float total = 0.0f;
    HIP_TRY(hipEventElapsedTime(&total, start, end));
    *ms = total / (float)repeats;
    return RAYRS_OK;
    })
}

int rayrs_probe_directions(uint64_t seed, uint64_t index_base, uint64_t n, uint32_t samples, double* out) {
    RAYRS_GUARDED({
    if (!out) return RAYRS_INVALID_ARG;
    for (uint64_t i = 0; i < n; i++)
        for (uint32_t s = 0; s < samples; s++) probe_sample_direction(seed, index_base + i, s, out + (i * samples + s) * 3u);
    return RAYRS_OK;
    })
}

int rayrs_sh_basis(const double* direction, uint64_t m, double* out) {
    RAYRS_GUARDED({
    if (!direction || !out) return RAYRS_INVALID_ARG;
    for (uint64_t k = 0; k < m; k++) sh_basis(direction[3u * k], direction[3u * k + 1u], direction[3u * k + 2u], out + SH_COEFFS * k);
    return RAYRS_OK;
    })
}

}  // extern "C"
