// film.hip -- the progressive film (include/rayrs_hip.h rayrs_film_*): the kernel that adds a pass's chunk sums to the
// film's records in place of the resolve kernel, the noise / NaN / negative counts over the records, and the frame read
// from them.  All three stream through memory once; none uses LDS.  The path kernels know nothing of a film: they see a
// sample window that does not start at 0 (layout.h RenderDev::sample0).
#include <hip/hip_runtime.h>

#include "../../include/rayrs_hip.h"
#include "film.h"

namespace rayrs {

namespace {
constexpr uint32_t ITEM_STRIDE = 64u * 3u;  // doubles between a pixel's sums of consecutive chunks (64 items of a tile each)
constexpr uint32_t UNROLL = 8;              // chunk sums a lane requests before it adds the first: 24 loads in flight

struct Rec {
    double x, y, z, s1, s2;
};

// the next chunk sum (cx, cy, cz) in chunk order; S1 and S2 take the channel sum of a full chunk, unfused
__device__ __forceinline__ void add_chunk(Rec& r, double cx, double cy, double cz, bool full) {
    r.x += cx, r.y += cy, r.z += cz;
    if (full) {
        const double c = (cx + cy) + cz;
        r.s1 += c;
        r.s2 += c * c;
    }
}

// The converged predicate of include/rayrs_hip.h on a pixel's S1 and S2 and its tile's M full chunks, in the header's
// operation order: is the pixel unconverged?  A non-finite one is neither that nor converged.
__device__ __forceinline__ bool pixel_unconverged(double s1, double s2, double m, double tau2, bool& nonfinite) {
    nonfinite = !(__builtin_isfinite(s1) && __builtin_isfinite(s2));
    const double s11 = s1 * s1;
    const bool converged = m >= 2.0 && m * s2 - s11 <= ((tau2 * s11)) * (m - 1.0);
    return !nonfinite && !converged;
}
}  // namespace

// One lane per pixel of the rank's tiles lt0 .. lt0 + n_lt - 1, as resolve_kernel indexes them: a wave holds one tile, so
// per chunk its lanes read 64 consecutive 24-byte item sums, and per record plane 512 consecutive bytes.
__global__ void __launch_bounds__(256) film_accumulate_kernel(CameraDev cam, RenderDev rp, FilmPassDev fp, uint32_t lt0, uint32_t n_lt) {
    const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (uint64_t)n_lt * 64u) return;
    const uint32_t pit = (uint32_t)(idx & 63u);
    const uint32_t lt = lt0 + (uint32_t)(idx >> 6);
    TilePixel px = tile_pixel(share_of(rp), lt, pit);
    uint32_t n_before = rp.sample0;
    bool first = fp.first != 0u;
    if (rp.tile_list) {  // the pass's tile lt, and what it holds: an empty tile's first chunk sum is assigned
        const TileRef t = rp.tile_list[lt];
        px = pixel_of_tile(share_of(rp), t.tile, pit, px.in_share), n_before = t.samples, first = t.samples == 0u;
    }
    if (!px.in_share || px.row >= cam.H || px.col >= cam.W) return;  // padding of an edge tile: its record stays zero
    double* rec = fp.rec + (size_t)px.tile * FILM_TILE_DOUBLES + pit;
    const double* src = rp.partial + ((((size_t)lt * rp.nchunks) * 64u + pit) - rp.partial_item0) * 3;
    const uint32_t n = rp.nchunks, full = fp.full_chunks;
    Rec r;
    uint32_t k = 0;
    if (first) {  // the first chunk sum a pixel ever gets is assigned, as resolve_kernel's (a -0 stays -0)
        r.x = src[0], r.y = src[1], r.z = src[2];
        const double c = (r.x + r.y) + r.z;
        r.s1 = full ? c : 0.0;
        r.s2 = full ? c * c : 0.0;
        src += ITEM_STRIDE;
        k = 1;
    } else {
        r.x = rec[FILM_SX * 64u], r.y = rec[FILM_SY * 64u], r.z = rec[FILM_SZ * 64u];
        r.s1 = rec[FILM_S1 * 64u], r.s2 = rec[FILM_S2 * 64u];
    }
    for (; k + UNROLL <= full; k += UNROLL, src += UNROLL * ITEM_STRIDE) {
        double c[UNROLL][3];
#pragma unroll
        for (uint32_t u = 0; u < UNROLL; u++) {
            c[u][0] = src[u * ITEM_STRIDE], c[u][1] = src[u * ITEM_STRIDE + 1], c[u][2] = src[u * ITEM_STRIDE + 2];
        }
#pragma unroll
        for (uint32_t u = 0; u < UNROLL; u++) add_chunk(r, c[u][0], c[u][1], c[u][2], true);
    }
    for (; k < n; k++, src += ITEM_STRIDE) add_chunk(r, src[0], src[1], src[2], k < full);
    rec[FILM_SX * 64u] = r.x, rec[FILM_SY * 64u] = r.y, rec[FILM_SZ * 64u] = r.z;
    rec[FILM_S1 * 64u] = r.s1, rec[FILM_S2 * 64u] = r.s2;
    if (pit == 0u) fp.tile_n[px.tile] = n_before + rp.spp;  // (pixel 0 of a tile of the frame is in the image)
}

// One pass over the records of the rank's tiles.  Per lane the tests of main.rs:81-87 on the running sum and the
// converged predicate of include/rayrs_hip.h (no square root, no division: the count is exactly reproducible); per wave a
// ballot and a population count, and one atomic add per counter that has anything to add.
__global__ void __launch_bounds__(256) film_status_kernel(CameraDev cam, TileShare ts, const double* recs, const uint32_t* tile_n,
                                                          uint32_t c, double tau2, FilmCounts* counts) {
    const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t pit = (uint32_t)(idx & 63u);
    const TilePixel px = tile_pixel(ts, (uint32_t)(idx >> 6), pit);
    const uint32_t n_t = px.in_share ? tile_n[px.tile] : 0u;
    const double m = (double)(n_t / c);  // the tile's own full chunks
    bool nan = false, neg = false, unconverged = false, nonfinite = false;
    if (px.in_share && px.row < cam.H && px.col < cam.W) {
        const double* rec = recs + (size_t)px.tile * FILM_TILE_DOUBLES + pit;
        const double x = rec[FILM_SX * 64u], y = rec[FILM_SY * 64u], z = rec[FILM_SZ * 64u];
        nan = x != x || y != y || z != z;        // main.rs:81
        neg = x < 0.0 || y < 0.0 || z < 0.0;    // main.rs:85
        unconverged = pixel_unconverged(rec[FILM_S1 * 64u], rec[FILM_S2 * 64u], m, tau2, nonfinite);
    }
    const unsigned long long b_nan = __ballot(nan), b_neg = __ballot(neg), b_unc = __ballot(unconverged), b_nf = __ballot(nonfinite);
    if ((threadIdx.x & 63u) == 0u) {
        if (b_nan) atomicAdd(&counts->nan_pixels, (unsigned long long)__popcll(b_nan));
        if (b_neg) atomicAdd(&counts->neg_pixels, (unsigned long long)__popcll(b_neg));
        if (b_unc) atomicAdd(&counts->unconverged, (unsigned long long)__popcll(b_unc));
        if (b_nf) atomicAdd(&counts->nonfinite, (unsigned long long)__popcll(b_nf));
        if (n_t) atomicMax(&counts->max_samples, n_t);
    }
}

// The frame as it stands: one lane per pixel in image order, so that the frame is written in whole lines; a lane reads
// its record's three sums where its tile keeps them (eight lanes share a 64-byte run of a plane).
__global__ void __launch_bounds__(256) film_read_kernel(CameraDev cam, uint32_t tiles_x, const double* recs, const uint32_t* tile_n,
                                                        uint32_t out_format, void* out) {
    const uint64_t pix = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= (uint64_t)cam.W * cam.H) return;
    const uint32_t row = (uint32_t)(pix / cam.W), col = (uint32_t)(pix % cam.W);
    const uint32_t tile = (row >> 3) * tiles_x + (col >> 3);
    const double* rec = recs + (size_t)tile * FILM_TILE_DOUBLES + ((row & 7u) * 8u + (col & 7u));
    const uint32_t n_t = tile_n[tile];
    const double inv_n = n_t ? 1.0 / (double)n_t : 0.0;  // (a tile without samples holds zeros: +0)
    const double x = rec[FILM_SX * 64u] * inv_n, y = rec[FILM_SY * 64u] * inv_n, z = rec[FILM_SZ * 64u] * inv_n;  // main.rs:89
    if (out_format == RAYRS_OUT_F64) {
        double* dst = reinterpret_cast<double*>(out) + pix * 3;
        dst[0] = x, dst[1] = y, dst[2] = z;
    } else {
        float* dst = reinterpret_cast<float*>(out) + pix * 3;  // image.rs:224-229
        dst[0] = (float)x, dst[1] = (float)y, dst[2] = (float)z;
    }
}

// The tiles an adaptive pass samples.  One wave per tile of the share, reading the records as film_status_kernel does and
// the same predicate with the tile's own M_t: one ballot says whether any in-image pixel is unconverged (a non-finite
// pixel is not, and padding never is).  The flag also needs room for n more samples below the cap.
__global__ void __launch_bounds__(256) film_select_kernel(CameraDev cam, TileShare ts, const double* recs, const uint32_t* tile_n,
                                                          uint32_t c, uint32_t n, uint32_t cap, double tau2, uint32_t all,
                                                          uint32_t* flags) {
    const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t pit = (uint32_t)(idx & 63u);
    const uint32_t lt = (uint32_t)(idx >> 6);
    const TilePixel px = tile_pixel(ts, lt, pit);  // (in_share is wave-uniform)
    const uint32_t n_t = px.in_share ? tile_n[px.tile] : 0u;
    const double m = (double)(n_t / c);
    bool unconverged = false, nonfinite;
    if (px.in_share && !all && px.row < cam.H && px.col < cam.W) {
        const double* rec = recs + (size_t)px.tile * FILM_TILE_DOUBLES + pit;
        unconverged = pixel_unconverged(rec[FILM_S1 * 64u], rec[FILM_S2 * 64u], m, tau2, nonfinite);
    }
    const unsigned long long b_unc = __ballot(unconverged);
    if (px.in_share && pit == 0u) flags[lt] = (all || (b_unc != 0ull && (uint64_t)n_t + n <= cap)) ? 1u : 0u;
}

// flags -> the list of (tile, N_t) in ascending tile order, by a scan: where a tile lands in the list, and with it the
// numbering of the pass's items, depends on the film's state alone, never on the order in which waves finish.  One
// workgroup walks the share 1024 tiles at a time: a ballot and a population count per wave, the sixteen wave totals
// through LDS, the running base in a register.  (65536 tiles, a 2048 x 2048 frame, are 64 steps.)
constexpr uint32_t COMPACT_THREADS = 1024;
__global__ void __launch_bounds__(COMPACT_THREADS) film_compact_kernel(TileShare ts, const uint32_t* flags, const uint32_t* tile_n,
                                                                       TileRef* list, FilmSelect* sel) {
    __shared__ uint32_t s_wave[COMPACT_THREADS / 64u];
    __shared__ uint32_t s_max;
    const uint32_t tid = threadIdx.x, wave = tid >> 6;
    if (tid == 0u) s_max = 0u;
    uint32_t base = 0u, most = 0u;
    for (uint32_t start = 0u; start < ts.n_local_tiles; start += COMPACT_THREADS) {
        const uint32_t lt = start + tid;
        const TilePixel px = tile_pixel(ts, lt, 0u);  // (the tile alone)
        const uint32_t n_t = px.in_share ? tile_n[px.tile] : 0u;
        const bool flagged = px.in_share && flags[lt] != 0u;
        most = n_t > most ? n_t : most;
        const unsigned long long b = __ballot(flagged);
        const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
        if ((tid & 63u) == 0u) s_wave[wave] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t before = 0u, total = 0u;
        for (uint32_t w = 0u; w < COMPACT_THREADS / 64u; w++) {
            const uint32_t v = s_wave[w];
            before += w < wave ? v : 0u;
            total += v;
        }
        if (flagged) {  // (base + before + below < the flagged tiles so far <= n_local_tiles: inside the list)
            TileRef t;
            t.tile = px.tile, t.samples = n_t;
            list[base + before + below] = t;
        }
        base += total;
        __syncthreads();
    }
    atomicMax(&s_max, most);
    __syncthreads();
    if (tid == 0u) sel->n_active = base, sel->max_samples = s_max;
}

hipError_t launch_film_accumulate(const CameraDev& cam, const RenderDev& rp, const FilmPassDev& fp, uint32_t lt0, uint32_t n_lt,
                                  hipStream_t stream) {
    const uint64_t n = (uint64_t)n_lt * 64u;
    if (n == 0 || rp.nchunks == 0) return hipSuccess;
    hipLaunchKernelGGL(film_accumulate_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream, cam, rp, fp, lt0, n_lt);
    return hipGetLastError();
}

hipError_t launch_film_status(const CameraDev& cam, const TileShare& ts, const double* rec, const uint32_t* tile_n, uint32_t c,
                              double tau2, FilmCounts* counts, hipStream_t stream) {
    const uint64_t n = (uint64_t)ts.n_local_tiles * 64u;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(film_status_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream, cam, ts, rec, tile_n, c, tau2, counts);
    return hipGetLastError();
}

hipError_t launch_film_read(const CameraDev& cam, uint32_t tiles_x, const double* rec, const uint32_t* tile_n, uint32_t out_format,
                            void* out, hipStream_t stream) {
    const uint64_t n = (uint64_t)cam.W * cam.H;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(film_read_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream, cam, tiles_x, rec, tile_n,
                       out_format, out);
    return hipGetLastError();
}

hipError_t launch_film_select(const CameraDev& cam, const TileShare& ts, const double* rec, const uint32_t* tile_n, uint32_t c,
                              uint32_t n, uint32_t cap, double tau2, uint32_t all, uint32_t* flags, TileRef* list, FilmSelect* sel,
                              hipStream_t stream) {
    const uint64_t threads = (uint64_t)ts.n_local_tiles * 64u;
    if (threads) {
        hipLaunchKernelGGL(film_select_kernel, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, stream, cam, ts, rec, tile_n, c, n,
                           cap, tau2, all, flags);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(film_compact_kernel, dim3(1), dim3(COMPACT_THREADS), 0, stream, ts, flags, tile_n, list, sel);
    return hipGetLastError();
}

}  // namespace rayrs
