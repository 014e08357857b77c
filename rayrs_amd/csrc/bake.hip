// bake.hip -- the bake (include/rayrs_hip.h BAKE): progressive, adaptive radiance queries at fixed points.  Its wave kernels are
// radiance_direct_wave.h's wave without and with the sky, started per (entry, chunk) item of a pass's sample window
// (bake_kernels.h BakeStart); behind every launch, on the same stream, bake_accumulate_kernel adds the launch's chunk sums to the
// points' records.  The selection of an adaptive pass is a stream compaction over the points -- flag and count, scan the
// workgroups' counts, scatter -- whose result depends on the records alone.  No arithmetic of a sample is written here: a
// chunk's sum is the waves'.
#include <hip/hip_runtime.h>

#include "bake_kernels.h"
#include "device_path.h"
#include "launch_dispatch.h"
#include "radiance_direct_wave.h"

namespace rayrs {

template <bool COMPACT, bool EXACT, int KIND>
__global__ void __launch_bounds__(256) bake_direct_kernel(SceneDev sc, RadianceDev rd, BakeStartDev bs, LightsDev lights, LightSlotsDev slots) {
    extern __shared__ uint32_t lds_stack[];
    const CameraDev cam{};  // (read by LIT_START_PIXEL only: never here)
    direct_wave<COMPACT, EXACT>(BakeStart<KIND>{bs}, lane_stack(lds_stack, rd.spill, sc), sc, rd, lights, slots, NoSky{}, cam);
}

template <bool COMPACT, bool EXACT, int KIND>
__global__ void __launch_bounds__(256) bake_sky_kernel(SceneDev sc, RadianceDev rd, BakeStartDev bs, LightsDev lights, LightSlotsDev slots,
                                                       SkyDev sky) {
    extern __shared__ uint32_t lds_stack[];
    const CameraDev cam{};
    direct_wave<COMPACT, EXACT>(BakeStart<KIND>{bs}, lane_stack(lds_stack, rd.spill, sc), sc, rd, lights, slots, sky, cam);
}

namespace {

// The converged predicate of include/rayrs_hip.h NOISE on a point's S1 and S2 and its own M full chunks, in the header's
// operation order (film.hip pixel_unconverged, word for word): is the point unconverged?  A non-finite one is neither that nor
// converged.
__device__ __forceinline__ bool point_unconverged(double s1, double s2, double m, double tau2, bool& nonfinite) {
    nonfinite = !(__builtin_isfinite(s1) && __builtin_isfinite(s2));
    const double s11 = s1 * s1;
    const bool converged = m >= 2.0 && m * s2 - s11 <= ((tau2 * s11)) * (m - 1.0);
    return !nonfinite && !converged;
}

// SELECTION for point i (i < bk.n): room for n more samples below the cap, and unconverged at tau.
__device__ __forceinline__ bool point_taken(const BakeDev& bk, uint64_t i, uint32_t c, uint32_t n, uint32_t cap, double tau2, uint32_t& n_i) {
    n_i = bk.count[i];
    bool nonfinite;
    const bool unconverged = point_unconverged(bk.rec[BAKE_S1 * bk.n + i], bk.rec[BAKE_S2 * bk.n + i], (double)(n_i / c), tau2, nonfinite);
    return unconverged && (uint64_t)n_i + n <= cap;
}

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_down((int)v, off, 64);
        v = o > v ? o : v;
    }
    return v;  // (lane 0's)
}

}  // namespace

// One thread per entry of the launch.  A thread reads its entry's chunks consecutive 24-byte item sums in chunk order; per
// record plane a wave reads and writes 512 consecutive bytes on a uniform pass (a list's points are ascending, so nearly so).
// Plain vector stores; the launch's query total is added across the wave's lanes and by one atomic per wave.
__global__ void __launch_bounds__(256) bake_accumulate_kernel(RadianceDev rd, BakeStartDev bs, BakeDev bk, uint32_t full_chunks,
                                                              uint32_t has_queries, BakePassCounts* counts) {
    const uint32_t el = blockIdx.x * 256u + threadIdx.x;
    unsigned long long q = 0ull;
    if (el < rd.n) {
        uint32_t point, n_before;
        bake_entry(bs, bs.e0 + el, point, n_before);
        const double* src = rd.partial + (size_t)el * rd.chunks * 3u;
        double* rec = bk.rec + point;
        double x, y, z, s1, s2;
        uint32_t k = 0;
        if (n_before == 0u) {  // the first chunk sum a point ever gets is assigned, as the queries' resolve does (a -0 stays -0)
            x = src[0], y = src[1], z = src[2];
            const double cs = (x + y) + z;
            const bool full = full_chunks != 0u;
            s1 = full ? cs : 0.0;
            s2 = full ? cs * cs : 0.0;
            k = 1;
        } else {
            x = rec[BAKE_SX * bk.n], y = rec[BAKE_SY * bk.n], z = rec[BAKE_SZ * bk.n];
            s1 = rec[BAKE_S1 * bk.n], s2 = rec[BAKE_S2 * bk.n];
        }
        for (; k < rd.chunks; k++) {
            const double cx = src[3u * k], cy = src[3u * k + 1u], cz = src[3u * k + 2u];
            x += cx, y += cy, z += cz;
            if (k < full_chunks) {  // S1 and S2 take the channel sum of a full chunk, unfused
                const double cs = (cx + cy) + cz;
                s1 += cs;
                s2 += cs * cs;
            }
        }
        rec[BAKE_SX * bk.n] = x, rec[BAKE_SY * bk.n] = y, rec[BAKE_SZ * bk.n] = z;
        rec[BAKE_S1 * bk.n] = s1, rec[BAKE_S2 * bk.n] = s2;
        if (has_queries) {
            const uint32_t* pq = rd.partial_queries + (size_t)el * rd.chunks;
            for (uint32_t j = 0; j < rd.chunks; j++) q += pq[j];
            bk.queries[point] += q;
        }
        bk.count[point] = n_before + bs.spp;
    }
    unsigned long long sum = q;
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_down((int)(uint32_t)sum, off, 64);
        const uint32_t hi = (uint32_t)__shfl_down((int)(uint32_t)(sum >> 32), off, 64);
        sum += ((unsigned long long)hi << 32) | lo;
    }
    if ((threadIdx.x & 63u) == 0u && sum) atomicAdd(&counts->queries, sum);
}

// The select's first step, one thread per point: a ballot and a population count per wave, the workgroup's four wave totals
// through LDS, one word per workgroup.  The largest N_i + n among the taken points goes to sel by one atomic max per wave: a
// maximum, which no order of the waves changes.
__global__ void __launch_bounds__(BAKE_SELECT_THREADS) bake_select_count_kernel(BakeDev bk, uint32_t c, uint32_t n, uint32_t cap, double tau2,
                                                                                uint32_t* block_counts, BakeSelect* sel) {
    __shared__ uint32_t s_wave[BAKE_SELECT_THREADS / 64u];
    const uint64_t i = (uint64_t)blockIdx.x * BAKE_SELECT_THREADS + threadIdx.x;
    uint32_t n_i = 0u;
    const bool taken = i < bk.n && point_taken(bk, i, c, n, cap, tau2, n_i);
    const unsigned long long b = __ballot(taken);
    const uint32_t most = wave_max(taken ? n_i + n : 0u);
    if ((threadIdx.x & 63u) == 0u) {
        s_wave[threadIdx.x >> 6] = (uint32_t)__popcll(b);
        if (most) atomicMax(&sel->max_after, most);
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t total = 0u;
        for (uint32_t w = 0u; w < BAKE_SELECT_THREADS / 64u; w++) total += s_wave[w];
        block_counts[blockIdx.x] = total;
    }
}

// The second: the workgroups' counts become their exclusive prefix sums, in place.  One workgroup walks them 1024 at a time: an
// inclusive scan inside each wave by cross-lane moves, the sixteen wave totals through LDS, the running base in a register.
// (2^20 points are 4096 counts, four steps.)  The total is the list's length.
constexpr uint32_t BAKE_SCAN_THREADS = 1024;
__global__ void __launch_bounds__(BAKE_SCAN_THREADS) bake_select_scan_kernel(uint32_t* block_counts, uint32_t n_blocks, BakeSelect* sel) {
    __shared__ uint32_t s_wave[BAKE_SCAN_THREADS / 64u];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    uint32_t base = 0u;
    for (uint32_t start = 0u; start < n_blocks; start += BAKE_SCAN_THREADS) {
        const uint32_t at = start + tid;
        const uint32_t v = at < n_blocks ? block_counts[at] : 0u;
        uint32_t incl = v;
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t o = (uint32_t)__shfl_up((int)incl, off, 64);
            if (lane >= (uint32_t)off) incl += o;
        }
        if (lane == 63u) s_wave[wave] = incl;
        __syncthreads();
        uint32_t before = 0u, total = 0u;
        for (uint32_t w = 0u; w < BAKE_SCAN_THREADS / 64u; w++) {
            const uint32_t t = s_wave[w];
            before += w < wave ? t : 0u;
            total += t;
        }
        if (at < n_blocks) block_counts[at] = base + before + (incl - v);
        base += total;
        __syncthreads();
    }
    if (tid == 0u) sel->n_active = base;
}

// The third, on the first's grid: the predicate once more, and a taken point goes to the list at its workgroup's offset plus the
// taken points before it in the workgroup -- ascending point order, whatever order the workgroups run in.
__global__ void __launch_bounds__(BAKE_SELECT_THREADS) bake_select_scatter_kernel(BakeDev bk, uint32_t c, uint32_t n, uint32_t cap, double tau2,
                                                                                  const uint32_t* block_offsets, BakeRef* list) {
    __shared__ uint32_t s_wave[BAKE_SELECT_THREADS / 64u];
    const uint64_t i = (uint64_t)blockIdx.x * BAKE_SELECT_THREADS + threadIdx.x;
    const uint32_t wave = threadIdx.x >> 6;
    uint32_t n_i = 0u;
    const bool taken = i < bk.n && point_taken(bk, i, c, n, cap, tau2, n_i);
    const unsigned long long b = __ballot(taken);
    const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
    if ((threadIdx.x & 63u) == 0u) s_wave[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t before = 0u;
    for (uint32_t w = 0u; w < BAKE_SELECT_THREADS / 64u; w++) before += w < wave ? s_wave[w] : 0u;
    if (taken) {  // (offset + before + below < the taken points so far <= n: inside the list)
        BakeRef r;
        r.point = (uint32_t)i, r.samples = n_i;
        list[block_offsets[blockIdx.x] + before + below] = r;
    }
}

// One pass over the records.  Per lane the converged predicate with the point's own M_i; per wave a ballot and a population
// count, and one atomic add per counter that has anything to add (film_direct.hip film_direct_count_kernel's way).
__global__ void __launch_bounds__(256) bake_status_kernel(BakeDev bk, uint32_t c, double tau2, BakeCounts* counts) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    bool unconverged = false, nonfinite = false;
    uint32_t n_i = 0u;
    if (i < bk.n) {
        n_i = bk.count[i];
        unconverged = point_unconverged(bk.rec[BAKE_S1 * bk.n + i], bk.rec[BAKE_S2 * bk.n + i], (double)(n_i / c), tau2, nonfinite);
    }
    const unsigned long long b_unc = __ballot(unconverged), b_nf = __ballot(nonfinite);
    const uint32_t most = wave_max(n_i);
    if ((threadIdx.x & 63u) == 0u) {
        if (b_unc) atomicAdd(&counts->unconverged, (unsigned long long)__popcll(b_unc));
        if (b_nf) atomicAdd(&counts->nonfinite, (unsigned long long)__popcll(b_nf));
        if (most) atomicMax(&counts->max_samples, most);
    }
}

// include/rayrs_hip.h NOISE PLANE per point (denoise.hip film_noise_kernel's arithmetic); +infinity is selected, never computed.
__global__ void __launch_bounds__(256) bake_noise_kernel(BakeDev bk, uint32_t c_u, double* variance) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= bk.n) return;
    const double s1 = bk.rec[BAKE_S1 * bk.n + i], s2 = bk.rec[BAKE_S2 * bk.n + i];
    const uint32_t big_m = bk.count[i] / c_u;
    const double m = (double)big_m, c = (double)c_u;
    const double inf = __builtin_huge_val();
    double v = inf;
    if (big_m >= 2u && __builtin_isfinite(s1) && __builtin_isfinite(s2)) {
        const double d = m * s2 - s1 * s1;
        if (__builtin_isfinite(d)) v = d > 0.0 ? d / (((m * m) * (m - 1.0)) * (c * c)) : 0.0;
    }
    variance[i] = v;
}

// The values as they stand: running sum * (1.0 / N_i), the queries' resolve.
__global__ void __launch_bounds__(256) bake_read_kernel(BakeDev bk, double* radiance) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= bk.n) return;
    const uint32_t n_i = bk.count[i];
    const double inv = n_i ? 1.0 / (double)n_i : 0.0;  // (a point without samples holds zeros: +0)
    double* dst = radiance + i * 3u;
    dst[0] = bk.rec[BAKE_SX * bk.n + i] * inv, dst[1] = bk.rec[BAKE_SY * bk.n + i] * inv, dst[2] = bk.rec[BAKE_SZ * bk.n + i] * inv;
}

hipError_t launch_bake_wave(bool compact, const SceneDev& sc, const RadianceDev& rd, const BakeStartDev& bs, const LightsDev& lights,
                            const LightSlotsDev& slots, const SkyDev* sky, bool irradiance, int cu_count, hipStream_t stream) {
    if (rd.n == 0u) return hipSuccess;
    const uint32_t blocks = radiance_grid_blocks(rd, cu_count);
    return with_bools([&](auto C, auto E, auto P) {
        constexpr int KIND = decltype(P)::value ? LIT_START_POINT : LIT_START_RAY;
        if (sky) return launch_lane_stacks(&bake_sky_kernel<decltype(C)::value, decltype(E)::value, KIND>, blocks, sc.stack_lds, stream, sc, rd,
                                           bs, lights, slots, *sky);
        return launch_lane_stacks(&bake_direct_kernel<decltype(C)::value, decltype(E)::value, KIND>, blocks, sc.stack_lds, stream, sc, rd, bs,
                                  lights, slots);
    }, compact, sc.exact != 0u, irradiance);
}

hipError_t launch_bake_accumulate(const RadianceDev& rd, const BakeStartDev& bs, const BakeDev& bk, uint32_t full_chunks,
                                  uint32_t has_queries, BakePassCounts* counts, hipStream_t stream) {
    if (rd.n == 0u || rd.chunks == 0u) return hipSuccess;
    hipLaunchKernelGGL(bake_accumulate_kernel, dim3((rd.n + 255u) / 256u), dim3(256), 0, stream, rd, bs, bk, full_chunks, has_queries, counts);
    return hipGetLastError();
}

hipError_t launch_bake_select(const BakeDev& bk, uint32_t c, uint32_t n, uint32_t cap, double tau2, uint32_t* block_counts, BakeRef* list,
                              BakeSelect* sel, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(sel, 0, sizeof(BakeSelect), stream);
    if (e != hipSuccess || bk.n == 0u) return e;
    const uint32_t blocks = (uint32_t)bake_select_blocks(bk.n);  // (n < 2^32: below 2^24)
    hipLaunchKernelGGL(bake_select_count_kernel, dim3(blocks), dim3(BAKE_SELECT_THREADS), 0, stream, bk, c, n, cap, tau2, block_counts, sel);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(bake_select_scan_kernel, dim3(1), dim3(BAKE_SCAN_THREADS), 0, stream, block_counts, blocks, sel);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(bake_select_scatter_kernel, dim3(blocks), dim3(BAKE_SELECT_THREADS), 0, stream, bk, c, n, cap, tau2, block_counts, list);
    return hipGetLastError();
}

hipError_t launch_bake_status(const BakeDev& bk, uint32_t c, double tau2, BakeCounts* counts, hipStream_t stream) {
    if (bk.n == 0u) return hipSuccess;
    hipLaunchKernelGGL(bake_status_kernel, dim3((uint32_t)((bk.n + 255u) / 256u)), dim3(256), 0, stream, bk, c, tau2, counts);
    return hipGetLastError();
}

hipError_t launch_bake_noise(const BakeDev& bk, uint32_t c, double* variance, hipStream_t stream) {
    if (bk.n == 0u) return hipSuccess;
    hipLaunchKernelGGL(bake_noise_kernel, dim3((uint32_t)((bk.n + 255u) / 256u)), dim3(256), 0, stream, bk, c, variance);
    return hipGetLastError();
}

hipError_t launch_bake_read(const BakeDev& bk, double* radiance, hipStream_t stream) {
    if (bk.n == 0u) return hipSuccess;
    hipLaunchKernelGGL(bake_read_kernel, dim3((uint32_t)((bk.n + 255u) / 256u)), dim3(256), 0, stream, bk, radiance);
    return hipGetLastError();
}

}  // namespace rayrs
