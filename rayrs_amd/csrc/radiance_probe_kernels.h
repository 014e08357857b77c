// radiance_probe_kernels.h -- SH probes (include/rayrs_hip.h SH PROBES: rayrs_scene_probes and its _launch form): the start a
// probe call gives the direct and the group wave (the fourth beside QueryStart, FilmStart and BakeStart), what
// radiance_probe.hip's projection kernels are handed, and the launch wrappers.  The wave's scratch, the thresholds, the light
// table, the slots and the groups are the radiance queries' (radiance_kernels.h, radiance_lit_kernels.h,
// radiance_direct_kernels.h, radiance_sky_kernels.h, radiance_mesh_kernels.h, radiance_tree_kernels.h).
#pragma once
#include <hip/hip_runtime.h>

#include "layout.h"
#include "radiance_direct_kernels.h"
#include "radiance_mesh_kernels.h"
#include "radiance_probe_table.h"
#include "radiance_sky_kernels.h"
#include "radiance_tree_kernels.h"

namespace rayrs {

// A launch takes whole probes, n * S <= RADIANCE_LAUNCH_ITEMS, so S is at most that.
constexpr uint32_t PROBE_MAX_SAMPLES = (uint32_t)RADIANCE_LAUNCH_ITEMS;

// The projection's own buffer (rayrs_scene::Probes::d_chunks, allocated at the scene's first probe call): the sums C[k][ch] of
// PROBE_CHUNK_SLOTS (probe, chunk) pairs as 27 planes -- plane c = k * 3 + ch begins at double c * PROBE_CHUNK_SLOTS, so that a
// wave's 64 consecutive pairs write 512 contiguous bytes per plane -- and behind them one u32 query count per pair.  A FIXED
// bound: a launch whose pairs outnumber the slots is projected in rounds of PROBE_CHUNK_SLOTS consecutive pairs, and a probe
// whose chunks lie in two rounds carries its running sum from one to the next in the caller's `coeffs` (and `queries`).
constexpr uint32_t PROBE_CHUNK_SLOTS = 1u << 15;
constexpr uint32_t PROBE_PLANES = SH_COEFFS * 3u;
constexpr size_t PROBE_CHUNK_BYTES = (size_t)PROBE_CHUNK_SLOTS * (PROBE_PLANES * sizeof(double) + sizeof(uint32_t));

// One round of a launch's projection: the pairs pair0 .. pair0 + pairs - 1 of the launch's n probes, pair = probe * chunks +
// chunk in launch-local numbering.  partial and partial_queries are the wave's, one entry per (probe, sample): item = probe * S + s.
struct ProbeDev {
    uint32_t n;               // the launch's probes
    uint32_t samples;         // S
    uint32_t chunk, chunks;   // the CALL's c' and chunks per probe (the wave ran with one sample per item)
    uint32_t pair0, pairs;    // pairs <= PROBE_CHUNK_SLOTS
    uint64_t seed, index_base;  // index_base: the launch's first probe's
    const double* partial;
    const uint32_t* partial_queries;
    double* slots;            // PROBE_PLANES planes of PROBE_CHUNK_SLOTS
    uint32_t* slot_queries;   // PROBE_CHUNK_SLOTS
    double* coeffs;           // n * 9 * 3: the launch's probes'
    uint32_t* queries;        // n, or null = not wanted
};

#if defined(__HIPCC__)
// The probes' start of the four waves.  An item is (probe, sample) in launch-local numbering, item = probe * S + s: QueryStart's
// numbering at chunk = 1, chunks = S, which is what rd.chunk and rd.chunks hold for the wave.
struct ProbeStart {
    static constexpr int KIND = LIT_START_PROBE;
    static constexpr bool SKIPS = false;
    __device__ __forceinline__ unsigned long long n_items(const RadianceDev& rd) const { return (unsigned long long)rd.n * rd.samples; }
    __device__ __forceinline__ bool take(const RadianceDev& rd, const CameraDev&, uint32_t item, uint32_t& ray, uint32_t& s,
                                         uint32_t& s_end) const {
        ray = item / rd.samples;
        s = item - ray * rd.samples;
        s_end = s + 1u;
        return true;
    }
    // (never called: KIND is not LIT_START_PIXEL)
    __device__ __forceinline__ void pixel(const RadianceDev&, const CameraDev&, uint32_t, uint32_t& row, uint32_t& col) const {
        row = 0u, col = 0u;
    }
};
#endif

// The wave of a probe launch on a grid of at most cu_count * RADIANCE_BLOCKS_PER_CU workgroups: every item's L_s into rd.partial
// and its query count into rd.partial_queries.  rd.chunk = 1, rd.chunks = rd.samples, rd.a the launch's points, rd.b unread.
// tree != nullptr: the group wave with the tree's group; else mesh != nullptr: with the area group; else the direct wave, with
// the sky where with_sky (without it, an empty list: the unlit bits).  with_sky also picks the group wave's sky instance.
hipError_t launch_probe_wave(bool compact, const SceneDev& sc, const RadianceDev& rd, const LightsDev& lights, const LightSlotsDev& slots,
                             const MeshDev* mesh, const TreeDev* tree, const SkyDev& sky, bool with_sky, int cu_count, hipStream_t stream);
// Behind it on the same stream, one round: probe_project_kernel, a thread per pair (its direction made again from the key, the
// nine Y_k, 27 sums in sample order), then probe_gather_kernel, a thread per (probe of the round, plane or count) adding the
// round's chunks in chunk order and, at a probe's last chunk, scaling.
hipError_t launch_probe_project(const ProbeDev& pd, hipStream_t stream);

}  // namespace rayrs
