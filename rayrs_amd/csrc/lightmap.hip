// lightmap.hip -- the lightmap atlas (include/rayrs_hip.h LIGHTMAP ATLAS).  The owner pass: a lane per triangle, the walk of its
// candidates by the lane, by the wave or by the whole grid according to their number, one integer atomicMin per covered texel.
// The compaction in ascending texel order is bake.hip's selection over another predicate -- ballot and population count per
// wave, a scan of the workgroups' counts -- and its scatter is the record pass: a thread per texel forms the owner's edge
// functions again and writes the record at the texel's place in the list.  The assembly: a scatter and a dilation round over two
// planes.  No atomic on an f64, no scratch memory; the only LDS is the wave totals of the count, the scan and the record pass.
#include <hip/hip_runtime.h>

#include "lightmap_kernels.h"

namespace rayrs {

namespace {

// Candidate t of the triangle's box, row-major: covered -> owner = min(owner, k).
__device__ __forceinline__ void owner_try(const LightmapDev& lm, const LightmapTri& t, uint32_t k, uint32_t x, uint32_t y) {
    double w1, w2;
    if (lightmap_covers(t, x, y, w1, w2)) atomicMin(lm.owner + ((size_t)y * lm.w + x), k);  // (x < w, y < h: lightmap_span)
}

}  // namespace

// A wave takes 64 consecutive triangles at a time, a lane each.  Boxes of at most LIGHTMAP_LANE_MAX candidates -- all of them in
// a per-triangle unwrap -- are walked by their lanes side by side; the wave then goes through its triangles with up to
// LIGHTMAP_WAVE_MAX candidates one after the other, all lanes striding one box; a larger one is only noted in big_list.
__global__ void __launch_bounds__(LIGHTMAP_THREADS) lightmap_owner_kernel(LightmapDev lm, uint32_t* big_list, LightmapCount* count) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * LIGHTMAP_THREADS + threadIdx.x) >> 6;
    const uint64_t step = (uint64_t)gridDim.x * (LIGHTMAP_THREADS / 64u) * 64u;
    for (uint64_t base = wave * 64u; base < lm.m; base += step) {
        const uint64_t k64 = base + lane;
        const uint32_t k = (uint32_t)k64;
        uint32_t cnt = 0u;
        LightmapTri t = {};
        if (k64 < lm.m) {
            t = lightmap_setup(lm, k);
            cnt = t.bw * t.bh;  // (at most 2^28)
        }
        if (cnt != 0u && cnt <= LIGHTMAP_LANE_MAX) {
            uint32_t x = t.x0, y = t.y0;
            for (uint32_t i = 0u; i < cnt; i++) {
                owner_try(lm, t, k, x, y);
                if (++x == t.x0 + t.bw) x = t.x0, y++;
            }
        }
        unsigned long long mid = __ballot(cnt > LIGHTMAP_LANE_MAX && cnt <= LIGHTMAP_WAVE_MAX);
        while (mid) {
            const uint32_t src = (uint32_t)__builtin_ctzll(mid);
            mid &= mid - 1ull;
            const uint32_t kk = (uint32_t)base + src;  // (the same in every lane)
            const LightmapTri tt = lightmap_setup(lm, kk);
            const uint32_t n = tt.bw * tt.bh;
            for (uint32_t i = lane; i < n; i += 64u) owner_try(lm, tt, kk, tt.x0 + i % tt.bw, tt.y0 + i / tt.bw);
        }
        if (cnt > LIGHTMAP_WAVE_MAX) big_list[atomicAdd(&count->big, 1u)] = k;  // (a triangle is listed once: below m entries)
    }
}

// The listed triangles one after the other, the whole grid striding each one's candidates.
__global__ void __launch_bounds__(LIGHTMAP_THREADS) lightmap_owner_big_kernel(LightmapDev lm, const uint32_t* big_list,
                                                                               const LightmapCount* count) {
    const uint32_t n_big = count->big;
    const uint32_t tid = blockIdx.x * LIGHTMAP_THREADS + threadIdx.x, threads = gridDim.x * LIGHTMAP_THREADS;
    for (uint32_t e = 0u; e < n_big; e++) {
        const uint32_t k = big_list[e];
        const LightmapTri t = lightmap_setup(lm, k);
        const uint32_t n = t.bw * t.bh;  // (at most 2^28: n + threads does not wrap)
        for (uint32_t i = tid; i < n; i += threads) owner_try(lm, t, k, t.x0 + i % t.bw, t.y0 + i / t.bw);
    }
}

// The compaction's first step, a thread per texel: a ballot and a population count per wave, one word per workgroup.
__global__ void __launch_bounds__(LIGHTMAP_THREADS) lightmap_count_kernel(const uint32_t* owner, uint64_t texels, uint32_t* block_counts) {
    __shared__ uint32_t s_wave[LIGHTMAP_THREADS / 64u];
    const uint64_t i = (uint64_t)blockIdx.x * LIGHTMAP_THREADS + threadIdx.x;
    const bool owned = i < texels && owner[i] != LIGHTMAP_NO_OWNER;
    const unsigned long long b = __ballot(owned);
    if ((threadIdx.x & 63u) == 0u) s_wave[threadIdx.x >> 6] = (uint32_t)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t total = 0u;
        for (uint32_t w = 0u; w < LIGHTMAP_THREADS / 64u; w++) total += s_wave[w];
        block_counts[blockIdx.x] = total;
    }
}

// The second: the workgroups' counts become their exclusive prefix sums, in place (bake.hip bake_select_scan_kernel's way: one
// workgroup walks them 1024 at a time, an inclusive scan inside each wave by cross-lane moves, the sixteen wave totals through
// LDS, the running base in a register).  The total is the list's length: at most 2^28.
constexpr uint32_t LIGHTMAP_SCAN_THREADS = 1024;
__global__ void __launch_bounds__(LIGHTMAP_SCAN_THREADS) lightmap_scan_kernel(uint32_t* block_counts, uint32_t n_blocks, LightmapCount* count) {
    __shared__ uint32_t s_wave[LIGHTMAP_SCAN_THREADS / 64u];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    uint32_t base = 0u;
    for (uint32_t start = 0u; start < n_blocks; start += LIGHTMAP_SCAN_THREADS) {
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
        for (uint32_t w = 0u; w < LIGHTMAP_SCAN_THREADS / 64u; w++) {
            const uint32_t t = s_wave[w];
            before += w < wave ? t : 0u;
            total += t;
        }
        if (at < n_blocks) block_counts[at] = base + before + (incl - v);
        base += total;
        __syncthreads();
    }
    if (tid == 0u) count->n = base;
}

// The record pass, on the count's grid: an owned texel's place is its workgroup's offset plus the owned texels before it in the
// workgroup -- ascending texel order, whatever order the workgroups run in -- and its record is TEXEL RECORD's, the owner's w1,
// w2 and area2 formed again as the owner pass formed them.
__global__ void __launch_bounds__(LIGHTMAP_THREADS) lightmap_record_kernel(LightmapDev lm, const uint32_t* block_offsets, LightmapList list) {
    __shared__ uint32_t s_wave[LIGHTMAP_THREADS / 64u];
    const uint64_t texels = (uint64_t)lm.w * lm.h;
    const uint64_t i = (uint64_t)blockIdx.x * LIGHTMAP_THREADS + threadIdx.x;
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t k = i < texels ? lm.owner[i] : LIGHTMAP_NO_OWNER;
    const bool owned = k != LIGHTMAP_NO_OWNER;
    const unsigned long long b = __ballot(owned);
    const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
    if ((threadIdx.x & 63u) == 0u) s_wave[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t before = 0u;
    for (uint32_t w = 0u; w < LIGHTMAP_THREADS / 64u; w++) before += w < wave ? s_wave[w] : 0u;
    if (!owned) return;
    const size_t at = (size_t)block_offsets[blockIdx.x] + before + below;  // (below the owned texels so far <= n: inside the list)
    const LightmapTri t = lightmap_setup(lm, k);  // (k < m: the owner pass wrote it)
    double w1, w2;
    (void)lightmap_covers(t, (uint32_t)(i % lm.w), (uint32_t)(i / lm.w), w1, w2);
    const double b1 = w1 / t.area2, b2 = w2 / t.area2;
    const double b0 = (1.0 - b1) - b2;
    const uint32_t* tri = lm.idx + (size_t)k * 3u;
    const double* p0 = lm.verts + (size_t)tri[0] * 3u;  // (idx entries are below nv: checked on the host)
    const double* p1 = lm.verts + (size_t)tri[1] * 3u;
    const double* p2 = lm.verts + (size_t)tri[2] * 3u;
    const double* nrm = lm.normals + (size_t)k * 3u;
    list.index[at] = (uint32_t)i;
    for (uint32_t c = 0u; c < 3u; c++) {
        list.points[at * 3u + c] = (b0 * p0[c] + b1 * p1[c]) + b2 * p2[c];
        list.normals[at * 3u + c] = nrm[c];
    }
    list.bary[at * 3u] = b0, list.bary[at * 3u + 1u] = b1, list.bary[at * 3u + 2u] = b2;
}

// ASSEMBLY's scatter, a thread per list entry (the planes are zeroed before it).
__global__ void __launch_bounds__(LIGHTMAP_THREADS) lightmap_scatter_kernel(const uint32_t* index, uint64_t n, const double* values, uint32_t c,
                                                                             double* image, uint8_t* valid) {
    const uint64_t i = (uint64_t)blockIdx.x * LIGHTMAP_THREADS + threadIdx.x;
    if (i >= n) return;
    const size_t texel = index[i];  // (below w * h: the record pass wrote it)
    for (uint32_t ch = 0u; ch < c; ch++) image[texel * c + ch] = values[i * c + ch];
    valid[texel] = 1u;
}

// One round of dilation, a thread per texel, from one pair of planes into the other.
template <int C>
__global__ void __launch_bounds__(LIGHTMAP_THREADS) lightmap_dilate_kernel(const double* image_in, const uint8_t* valid_in, double* image_out,
                                                                            uint8_t* valid_out, uint32_t w, uint32_t h, uint32_t* changed) {
    const uint64_t i = (uint64_t)blockIdx.x * LIGHTMAP_THREADS + threadIdx.x;
    bool made = false;
    if (i < (uint64_t)w * h) {
        const uint32_t x = (uint32_t)(i % w), y = (uint32_t)(i / w);
        double s[C];
        uint8_t v = valid_in[i];
        if (v) {
#pragma unroll
            for (int ch = 0; ch < C; ch++) s[ch] = image_in[i * C + ch];
        } else {
            uint32_t cnt = 0u;
#pragma unroll
            for (int ch = 0; ch < C; ch++) s[ch] = 0.0;
            for (int dy = -1; dy <= 1; dy++) {
                for (int dx = -1; dx <= 1; dx++) {
                    const int64_t qx = (int64_t)x + dx, qy = (int64_t)y + dy;
                    if (qx < 0 || qy < 0 || qx >= (int64_t)w || qy >= (int64_t)h) continue;
                    const size_t q = (size_t)qy * w + (size_t)qx;  // (the centre is invalid: it skips itself)
                    if (!valid_in[q]) continue;
#pragma unroll
                    for (int ch = 0; ch < C; ch++) s[ch] = s[ch] + image_in[q * C + ch];
                    cnt++;
                }
            }
            if (cnt) {
                const double d = (double)cnt;
#pragma unroll
                for (int ch = 0; ch < C; ch++) s[ch] = s[ch] / d;
                v = 1u, made = true;
            }
        }
#pragma unroll
        for (int ch = 0; ch < C; ch++) image_out[i * C + ch] = s[ch];
        valid_out[i] = v;
    }
    const unsigned long long b = __ballot(made);
    if (b != 0ull && (threadIdx.x & 63u) == 0u) *changed = 1u;  // (every writer writes the same word)
}

hipError_t launch_lightmap_owner(const LightmapDev& lm, uint32_t* big_list, LightmapCount* count, hipStream_t stream) {
    const uint64_t texels = (uint64_t)lm.w * lm.h;
    hipError_t e = hipMemsetAsync(lm.owner, 0xFF, texels * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(count, 0, sizeof(LightmapCount), stream)) != hipSuccess || lm.m == 0u) return e;
    const uint64_t want = ((uint64_t)lm.m + LIGHTMAP_THREADS - 1u) / LIGHTMAP_THREADS;
    const uint32_t blocks = want < LIGHTMAP_OWNER_BLOCKS ? (uint32_t)want : LIGHTMAP_OWNER_BLOCKS;
    hipLaunchKernelGGL(lightmap_owner_kernel, dim3(blocks), dim3(LIGHTMAP_THREADS), 0, stream, lm, big_list, count);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(lightmap_owner_big_kernel, dim3(LIGHTMAP_BIG_BLOCKS), dim3(LIGHTMAP_THREADS), 0, stream, lm, big_list, count);
    return hipGetLastError();
}

hipError_t launch_lightmap_compact(const LightmapDev& lm, uint32_t* block_offsets, LightmapCount* count, hipStream_t stream) {
    const uint64_t texels = (uint64_t)lm.w * lm.h;
    const uint32_t blocks = lightmap_blocks(texels);
    hipLaunchKernelGGL(lightmap_count_kernel, dim3(blocks), dim3(LIGHTMAP_THREADS), 0, stream, lm.owner, texels, block_offsets);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lightmap_scan_kernel, dim3(1), dim3(LIGHTMAP_SCAN_THREADS), 0, stream, block_offsets, blocks, count);
    return hipGetLastError();
}

hipError_t launch_lightmap_records(const LightmapDev& lm, const uint32_t* block_offsets, const LightmapList& list, hipStream_t stream) {
    const uint32_t blocks = lightmap_blocks((uint64_t)lm.w * lm.h);
    hipLaunchKernelGGL(lightmap_record_kernel, dim3(blocks), dim3(LIGHTMAP_THREADS), 0, stream, lm, block_offsets, list);
    return hipGetLastError();
}

hipError_t launch_lightmap_scatter(const uint32_t* index, uint64_t n, const double* values, uint32_t c, uint64_t texels, double* image,
                                   uint8_t* valid, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(image, 0, texels * c * sizeof(double), stream);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(valid, 0, texels, stream)) != hipSuccess || n == 0u) return e;
    hipLaunchKernelGGL(lightmap_scatter_kernel, dim3(lightmap_blocks(n)), dim3(LIGHTMAP_THREADS), 0, stream, index, n, values, c, image, valid);
    return hipGetLastError();
}

hipError_t launch_lightmap_dilate(const double* image_in, const uint8_t* valid_in, double* image_out, uint8_t* valid_out, uint32_t w,
                                  uint32_t h, uint32_t c, uint32_t* changed, hipStream_t stream) {
    const dim3 grid(lightmap_blocks((uint64_t)w * h)), block(LIGHTMAP_THREADS);
    switch (c) {
        case 1: hipLaunchKernelGGL(lightmap_dilate_kernel<1>, grid, block, 0, stream, image_in, valid_in, image_out, valid_out, w, h, changed); break;
        case 2: hipLaunchKernelGGL(lightmap_dilate_kernel<2>, grid, block, 0, stream, image_in, valid_in, image_out, valid_out, w, h, changed); break;
        case 3: hipLaunchKernelGGL(lightmap_dilate_kernel<3>, grid, block, 0, stream, image_in, valid_in, image_out, valid_out, w, h, changed); break;
        case 4: hipLaunchKernelGGL(lightmap_dilate_kernel<4>, grid, block, 0, stream, image_in, valid_in, image_out, valid_out, w, h, changed); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace rayrs
