// denoise.hip -- the film's per-pixel noise plane and the two a-trous filters (include/rayrs_hip.h NOISE PLANE, DENOISER
// and GUIDED FILTER).  No kernel here is part of a render.  All four stream through memory; none uses LDS.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/rayrs_hip.h"
#include "../../include/rayrs_numeric.h"
#include "film.h"
#include "denoise_kernels.h"

namespace rayrs {

// One wave per 8x8 tile of the share, one lane per pixel, as the film kernels map them: the S1 and the S2 plane of a tile
// are one 512-byte run each.  The variance of Y = (r + g) + b of the frame rayrs_film_read returns, by batch means over
// the tile's own M = N_t / c full chunks, in the header's order; +infinity is selected, never computed.
__global__ void __launch_bounds__(256) film_noise_kernel(FilmNoiseDev n) {
    const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t pit = (uint32_t)(idx & 63u);
    const TilePixel px = tile_pixel(n.share, (uint32_t)(idx >> 6), pit);
    if (!px.in_share || px.row >= n.h || px.col >= n.w) return;  // outside the share, or padding of an edge tile
    const double* rec = n.rec + (size_t)px.tile * FILM_TILE_DOUBLES + pit;
    const double s1 = rec[FILM_S1 * 64u], s2 = rec[FILM_S2 * 64u];
    const uint32_t big_m = n.tile_n[px.tile] / n.c;
    const double m = (double)big_m, c = (double)n.c;
    const double inf = __builtin_huge_val();
    double v = inf;
    if (big_m >= 2u && __builtin_isfinite(s1) && __builtin_isfinite(s2)) {
        const double d = m * s2 - s1 * s1;
        if (__builtin_isfinite(d)) v = d > 0.0 ? d / (((m * m) * (m - 1.0)) * (c * c)) : 0.0;
    }
    n.variance[(size_t)px.row * n.w + px.col] = v;
}

// Level 0's records from a colour frame and a variance plane, one lane per pixel.
__global__ void __launch_bounds__(256) guided_pack_kernel(const double* color, const double* variance, GuidedRec* out, uint64_t npix) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    GuidedRec r;
    r.cx = color[3 * p], r.cy = color[3 * p + 1], r.cz = color[3 * p + 2], r.v = variance[p];
    out[p] = r;
}

// One level of the edge-avoiding a-trous filter (Dammertz et al. 2010), in its two modes, exactly as include/rayrs_hip.h
// DENOISER and GUIDED FILTER state them: 5 x 5 taps `step` pixels apart, the weight of a tap the B3-spline's times
// rr_exp(-e), e the feature distances and the mode's own last term in the header's operation order.  One lane per pixel, a
// wave 64 consecutive pixels of a row; neighbouring rows and the next level's wider taps meet in L2, not in LDS.
//   plain  (AtrousDev): a pixel is three doubles of a 24-byte colour plane (a wave's 25 colour reads are 25 runs of 1536
//                       bytes); the last term is the colour distance times kc.
//   guided (GuidedDev): a pixel's colour and variance are one 32-byte record; the 3 x 3 prefilter of the variance at
//                       distance 1 comes first, a tap's luminance distance is divided by the prefiltered variance, and the
//                       variance is carried through with the squared weights.
constexpr uint32_t ATROUS_BX = 64, ATROUS_BY = 4;

namespace {
__device__ __forceinline__ bool finite3(double x, double y, double z) {
    return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z);
}
__device__ __forceinline__ double dist2(double ax, double ay, double az, double bx, double by, double bz) {
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}
// pixel q of the level's input (the plain filter carries no variance: v is never read there)
__device__ __forceinline__ GuidedRec fetch(const AtrousDev& a, size_t q) {
    return GuidedRec{a.color[3 * q], a.color[3 * q + 1], a.color[3 * q + 2], 0.0};
}
__device__ __forceinline__ GuidedRec fetch(const GuidedDev& a, size_t q) { return a.in[q]; }

template <bool GUIDED>
__device__ __forceinline__ void atrous_level(const std::conditional_t<GUIDED, GuidedDev, AtrousDev>& a) {
    const uint32_t x = blockIdx.x * ATROUS_BX + threadIdx.x;
    const uint32_t y = blockIdx.y * ATROUS_BY + threadIdx.y;
    if (x >= a.w || y >= a.h) return;
    const size_t p = (size_t)y * a.w + x;
    const GuidedRec rp = fetch(a, p);
    double ox = rp.cx, oy = rp.cy, oz = rp.cz, ov = rp.v;
    if (finite3(rp.cx, rp.cy, rp.cz)) {
        double r = 0.0, yp = 0.0;  // (guided) kv over the prefiltered variance, and the pixel's luminance
        if constexpr (GUIDED) {
            // the prefiltered variance: adjacent pixels, whatever the level's step
            constexpr double g[2] = {0.5, 0.25};
            double gs = 0.0, gw = 0.0;
#pragma unroll
            for (int dy = -1; dy <= 1; dy++) {
                const int qy = (int)y + dy;
                if (qy < 0 || qy >= (int)a.h) continue;
#pragma unroll
                for (int dx = -1; dx <= 1; dx++) {
                    const int qx = (int)x + dx;
                    if (qx < 0 || qx >= (int)a.w) continue;
                    const GuidedRec rq = fetch(a, (size_t)qy * a.w + (uint32_t)qx);
                    if (!finite3(rq.cx, rq.cy, rq.cz)) continue;
                    if (!(rq.v >= 0.0)) continue;
                    const double wt = g[dy < 0 ? -dy : dy] * g[dx < 0 ? -dx : dx];
                    gs += rq.v * wt;
                    gw += wt;
                }
            }
            r = gw == 0.0 ? 0.0 : a.kv / (gs / gw + RAYRS_GUIDED_EPS);
            yp = (rp.cx + rp.cy) + rp.cz;
        }
        const bool has_n = a.normal != nullptr, has_a = a.albedo != nullptr, has_z = a.depth != nullptr;  // (uniform)
        double npx = 0.0, npy = 0.0, npz = 0.0, apx = 0.0, apy = 0.0, apz = 0.0, zp = 0.0;
        if (has_n) npx = a.normal[3 * p], npy = a.normal[3 * p + 1], npz = a.normal[3 * p + 2];
        if (has_a) apx = a.albedo[3 * p], apy = a.albedo[3 * p + 1], apz = a.albedo[3 * p + 2];
        if (has_z) zp = a.depth[p];
        constexpr double h[3] = {0.375, 0.25, 0.0625};
        double nx = 0.0, ny = 0.0, nz = 0.0, den = 0.0, vs = 0.0;
        const int step = (int)a.step;  // at most 2^15: y + 2 * step stays far inside an int
#pragma unroll
        for (int dy = -2; dy <= 2; dy++) {
            const int qy = (int)y + dy * step;
            if (qy < 0 || qy >= (int)a.h) continue;
#pragma unroll
            for (int dx = -2; dx <= 2; dx++) {
                const int qx = (int)x + dx * step;
                if (qx < 0 || qx >= (int)a.w) continue;
                const size_t q = (size_t)qy * a.w + (uint32_t)qx;
                const GuidedRec rq = fetch(a, q);
                if (!finite3(rq.cx, rq.cy, rq.cz)) continue;
                if constexpr (GUIDED)
                    if (!(rq.v >= 0.0)) continue;
                // an absent plane's term is +0: every term is >= +0 or NaN, so adding it changes no bit of e
                double dn = 0.0, da = 0.0, dz = 0.0;
                if (has_n) dn = dist2(npx, npy, npz, a.normal[3 * q], a.normal[3 * q + 1], a.normal[3 * q + 2]);
                if (has_a) da = dist2(apx, apy, apz, a.albedo[3 * q], a.albedo[3 * q + 1], a.albedo[3 * q + 2]);
                if (has_z) {
                    const double zq = a.depth[q];
                    dz = (zp - zq) * (zp - zq);
                }
                double last;  // the mode's own term of e
                if constexpr (GUIDED) {
                    const double dl = yp - ((rq.cx + rq.cy) + rq.cz);
                    last = (dl * dl) * r;
                } else {
                    last = dist2(rp.cx, rp.cy, rp.cz, rq.cx, rq.cy, rq.cz) * a.kc;
                }
                const double e = ((dn * a.kn + da * a.ka) + dz * a.kz) + last;
                if (!__builtin_isfinite(e)) continue;
                const double w = (h[dy < 0 ? -dy : dy] * h[dx < 0 ? -dx : dx]) * rr_exp(-e);
                nx += rq.cx * w, ny += rq.cy * w, nz += rq.cz * w;
                den += w;
                if constexpr (GUIDED) {
                    const double ww = w * w;
                    vs += ww == 0.0 ? 0.0 : rq.v * ww;  // (0 x infinity)
                }
            }
        }
        // (den == 0: the pixel's own features are NaN)
        if constexpr (GUIDED) {
            const double den2 = den * den;
            if (den != 0.0 && den2 != 0.0) ox = nx / den, oy = ny / den, oz = nz / den, ov = vs / den2;
        } else {
            if (den != 0.0) ox = nx / den, oy = ny / den, oz = nz / den;
        }
    }
    void* out;
    if constexpr (GUIDED) {
        if (!a.last) {
            a.out_rec[p] = GuidedRec{ox, oy, oz, ov};
            return;
        }
        out = a.out_color;
    } else {
        out = a.out;
    }
    if (a.out_f32) {
        float* dst = reinterpret_cast<float*>(out) + 3 * p;  // image.rs:224-229
        dst[0] = (float)ox, dst[1] = (float)oy, dst[2] = (float)oz;
    } else {
        double* dst = reinterpret_cast<double*>(out) + 3 * p;
        dst[0] = ox, dst[1] = oy, dst[2] = oz;
    }
    if constexpr (GUIDED)
        if (a.out_variance) a.out_variance[p] = ov;
}
}  // namespace

__global__ void __launch_bounds__(ATROUS_BX * ATROUS_BY) atrous_kernel(AtrousDev a) { atrous_level<false>(a); }
__global__ void __launch_bounds__(ATROUS_BX * ATROUS_BY) guided_atrous_kernel(GuidedDev a) { atrous_level<true>(a); }

hipError_t launch_film_noise(const FilmNoiseDev& n, hipStream_t stream) {
    const uint64_t threads = (uint64_t)n.share.n_local_tiles * 64u;
    if (threads == 0) return hipSuccess;
    hipLaunchKernelGGL(film_noise_kernel, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, stream, n);
    return hipGetLastError();
}

hipError_t launch_guided_pack(const double* color, const double* variance, GuidedRec* out, uint32_t w, uint32_t h, hipStream_t stream) {
    const uint64_t npix = (uint64_t)w * h;
    if (npix == 0) return hipSuccess;
    hipLaunchKernelGGL(guided_pack_kernel, dim3((uint32_t)((npix + 255) / 256)), dim3(256), 0, stream, color, variance, out, npix);
    return hipGetLastError();
}

hipError_t launch_atrous(const AtrousDev& a, hipStream_t stream) {
    if (a.w == 0u || a.h == 0u) return hipSuccess;
    // (a.h <= 65535: the grid's y dimension holds it)
    hipLaunchKernelGGL(atrous_kernel, dim3((a.w + ATROUS_BX - 1u) / ATROUS_BX, (a.h + ATROUS_BY - 1u) / ATROUS_BY),
                       dim3(ATROUS_BX, ATROUS_BY), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_guided_atrous(const GuidedDev& g, hipStream_t stream) {
    if (g.w == 0u || g.h == 0u) return hipSuccess;
    // (g.h <= 65535: the grid's y dimension holds it)
    hipLaunchKernelGGL(guided_atrous_kernel, dim3((g.w + ATROUS_BX - 1u) / ATROUS_BX, (g.h + ATROUS_BY - 1u) / ATROUS_BY),
                       dim3(ATROUS_BX, ATROUS_BY), 0, stream, g);
    return hipGetLastError();
}

}  // namespace rayrs
