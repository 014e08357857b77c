// bake_kernels.h -- the bake (include/rayrs_hip.h BAKE: rayrs_bake_*): a device-resident accumulation buffer over the caller's
// rays or points.  Its records, the start a bake pass gives the direct and the group wave (the third beside QueryStart and
// FilmStart), what bake.hip's kernels are handed, and their launch wrappers.  The scratch, the thresholds, the light table and the
// slots are the radiance queries' (radiance_kernels.h, radiance_lit_kernels.h, radiance_direct_kernels.h).
#pragma once
#include <hip/hip_runtime.h>

#include "layout.h"
#include "radiance_sky_kernels.h"

namespace rayrs {

// One record per point, as planes over the bake's n points -- plane p begins at double p * n -- so that a wave's 64 consecutive
// points read and write 512 contiguous bytes per plane: the running sum of the point's chunk sums (x, y, z), and S1 and S2, the
// sum and the sum of squares of the channel sums y_k = (x_k + y_k) + z_k of its FULL chunks (the film's record, film.h).  Beside
// them, per point, the closest-hit queries of its paths in 64 bits and its sample count N_i.
constexpr uint32_t BAKE_PLANES = 5;
constexpr uint32_t BAKE_SX = 0, BAKE_SY = 1, BAKE_SZ = 2, BAKE_S1 = 3, BAKE_S2 = 4;

struct BakeDev {
    double* rec;                  // BAKE_PLANES * n
    unsigned long long* queries;  // n
    uint32_t* count;              // n: N_i
    uint64_t n;
};

// An entry of an adaptive pass's list: a selected point and the samples it holds, read in one 8-byte load.
struct BakeRef {
    uint32_t point, samples;
};

// One launch of a pass: the pass's entries e0 .. e0 + rd.n - 1, which are the list's (each point from the N_i the list holds) or,
// list == nullptr, the points e0 .. themselves (each from its own count).  RadianceDev carries the rest: n = the launch's
// points, chunk = c, chunks = the pass's chunks per point, a and b the bake's WHOLE arrays, index_base the bake's, and the scratch.
struct BakeStartDev {
    const BakeRef* list;
    const uint32_t* count;
    uint32_t e0, spp;  // the window of a point: samples N_i .. N_i + spp - 1
};

#if defined(__HIPCC__)
// The point of entry e of the pass and the samples it holds.
__device__ __forceinline__ void bake_entry(const BakeStartDev& bs, uint32_t e, uint32_t& point, uint32_t& n_before) {
    if (bs.list != nullptr) {
        const unsigned long long t = *reinterpret_cast<const unsigned long long*>(bs.list + e);
        point = (uint32_t)t, n_before = (uint32_t)(t >> 32);
    } else {
        point = e, n_before = bs.count[e];
    }
}

// The bake's start of radiance_direct_wave.h's and radiance_group_wave.h's waves.  An item is (entry, chunk of the pass) in
// launch-local numbering, item = entry * chunks + chunk; a lane's `ray` is the point's index in the bake, so the sample's RNG key
// is rr_path_key(seed, index_base + point, s): the key of the one-point query the contract names.
template <int START>
struct BakeStart {
    static constexpr int KIND = START;
    static constexpr bool SKIPS = false;
    const BakeStartDev& bs;  // (the kernel's argument)
    __device__ __forceinline__ unsigned long long n_items(const RadianceDev& rd) const { return (unsigned long long)rd.n * rd.chunks; }
    __device__ __forceinline__ bool take(const RadianceDev& rd, const CameraDev&, uint32_t item, uint32_t& ray, uint32_t& s,
                                         uint32_t& s_end) const {
        const uint32_t el = item / rd.chunks;
        const uint32_t k = item - el * rd.chunks;
        uint32_t n_before;
        bake_entry(bs, bs.e0 + el, ray, n_before);
        const uint32_t w_end = n_before + bs.spp;  // (at most 2^30 - 1: the pass rules)
        s = n_before + k * rd.chunk;
        s_end = s + rd.chunk < w_end ? s + rd.chunk : w_end;
        return true;
    }
    // (never called: KIND is not LIT_START_PIXEL)
    __device__ __forceinline__ void pixel(const RadianceDev&, const CameraDev&, uint32_t, uint32_t& row, uint32_t& col) const {
        row = 0u, col = 0u;
    }
};
#endif

// What a pass's launches leave for the host beside the records: the closest-hit queries of its items.
struct BakePassCounts {
    unsigned long long queries;
};

// What bake_select leaves for the host, read back as ONE 8-byte word per pass: the list's length, and the largest N_i + n among
// the selected points (0: none).
struct BakeSelect {
    uint32_t n_active, max_after;
};

struct BakeCounts {  // bake_status_kernel's counters, and the largest N_i
    unsigned long long unconverged, nonfinite;
    unsigned int max_samples, pad;
};

constexpr uint32_t BAKE_SELECT_THREADS = 256;  // points per workgroup of the flagging and the scatter
inline uint64_t bake_select_blocks(uint64_t n) { return (n + BAKE_SELECT_THREADS - 1u) / BAKE_SELECT_THREADS; }

// bake_direct_kernel (sky == nullptr) or bake_sky_kernel on a grid of at most cu_count * RADIANCE_BLOCKS_PER_CU workgroups: the
// chunk sums of the launch's items into rd.partial, their query counts into rd.partial_queries.  irradiance: LIT_START_POINT,
// else LIT_START_RAY.
hipError_t launch_bake_wave(bool compact, const SceneDev& sc, const RadianceDev& rd, const BakeStartDev& bs, const LightsDev& lights,
                            const LightSlotsDev& slots, const SkyDev* sky, bool irradiance, int cu_count, hipStream_t stream);
// Behind a launch on the same stream, one thread per entry of it: the entry's chunk sums added to its point's record in chunk
// order (a point without samples: the first one assigned), S1 and S2 from the first full_chunks chunks, queries_i += the
// items' counts (has_queries == 0: none were made, the scratch's counts are not read), N_i += bs.spp, and counts->queries += the
// launch's.
hipError_t launch_bake_accumulate(const RadianceDev& rd, const BakeStartDev& bs, const BakeDev& bk, uint32_t full_chunks,
                                  uint32_t has_queries, BakePassCounts* counts, hipStream_t stream);
// The points of an adaptive pass of n samples (include/rayrs_hip.h BAKE, SELECTION): list = the points with N_i + n <= cap that
// are unconverged at tau with M_i = N_i / c, in ascending order, and *sel.  block_counts: bake_select_blocks(n) words;
// list: n entries.
hipError_t launch_bake_select(const BakeDev& bk, uint32_t c, uint32_t n, uint32_t cap, double tau2, uint32_t* block_counts, BakeRef* list,
                              BakeSelect* sel, hipStream_t stream);
// counts += the unconverged and the non-finite points at tau, each with its own M_i; max_samples = the largest N_i
hipError_t launch_bake_status(const BakeDev& bk, uint32_t c, double tau2, BakeCounts* counts, hipStream_t stream);
// variance[i] = NOISE PLANE's formula on point i's S1, S2 and M_i
hipError_t launch_bake_noise(const BakeDev& bk, uint32_t c, double* variance, hipStream_t stream);
// radiance[i] = running sum * (1.0 / N_i); +0 for a point without samples
hipError_t launch_bake_read(const BakeDev& bk, double* radiance, hipStream_t stream);

}  // namespace rayrs
