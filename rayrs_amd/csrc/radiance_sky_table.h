// radiance_sky_table.h -- the sky as a light (include/rayrs_hip.h SKY SAMPLING): the table's layout, sky_sample and p_env, written
// once for the host calls (rayrs_scene_sky_sample, rayrs_scene_sky_density: radiance_sky_abi.cpp) and for radiance_sky.hip's
// kernel.  All f64, unfused, in the header's operation order; the elementary functions are rayrs_numeric.h's.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/rayrs_numeric.h"

#if defined(__HIPCC__)
#define SKY_HD __host__ __device__ static inline
#else
#define SKY_HD static inline
#endif

namespace rayrs {

// The table of a w x h map, one array of f64 (host: rayrs_scene::Sky::table; device: its copy):
//   M[h-1]            the inclusive prefix of the rows' sums R_i
//   C[h-1][w-1]       the inclusive prefix of A[i][.] along each row; R_i = C[i][w-2]
//   A[h-1][w-1]       the cells
// and beside it the sizes and T = M[h-2].  BY VALUE in the kernel arguments.
struct SkyDev {
    const double* table;
    uint32_t w, h;
    double T;
};
SKY_HD size_t sky_table_doubles(uint32_t w, uint32_t h) { return (size_t)(h - 1u) + 2u * (size_t)(h - 1u) * (w - 1u); }
SKY_HD const double* sky_M(const SkyDev& s) { return s.table; }
SKY_HD const double* sky_C(const SkyDev& s, uint32_t i) { return s.table + (s.h - 1u) + (size_t)i * (s.w - 1u); }
SKY_HD const double* sky_A(const SkyDev& s, uint32_t i) {
    return s.table + (s.h - 1u) + (size_t)(s.h - 1u) * (s.w - 1u) + (size_t)i * (s.w - 1u);
}

// The first index of the non-decreasing p[0 .. n-1] whose value exceeds t, or n - 1 if there is none: a binary search whose
// every read is inside the array (n >= 1).
SKY_HD uint32_t sky_first_above(const double* p, uint32_t n, double t) {
    uint32_t lo = 0u, hi = n - 1u;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (p[mid] > t) hi = mid;
        else lo = mid + 1u;
    }
    return lo;
}

// Rust `as usize` of a floor, then min with `last`: NaN and negatives are 0.
SKY_HD uint32_t sky_cell_index(double f, uint32_t last) {
    if (!(f > 0.0)) return 0u;
    if (f >= (double)last) return last;
    return (uint32_t)f;
}

// sky_sample(u1, u2): l_s into out[3].
SKY_HD void sky_sample(const SkyDev& s, double u1, double u2, double* out) {
    const uint32_t rows = s.h - 1u, cols = s.w - 1u;
    const double* M = sky_M(s);
    const double ty = u1 * s.T;
    const uint32_t i = sky_first_above(M, rows, ty);
    const double below_y = i > 0u ? M[i - 1u] : 0.0;
    const double* Ci = sky_C(s, i);
    const double Ri = Ci[cols - 1u];
    const double y = (double)i + (ty - below_y) / Ri;
    const double tx = u2 * Ri;
    const uint32_t j = sky_first_above(Ci, cols, tx);
    const double below_x = j > 0u ? Ci[j - 1u] : 0.0;
    const double x = (double)j + (tx - below_x) / sky_A(s, i)[j];
    const double theta = y / (double)(s.h - 1u) * RR_PI;
    const double phi = x / (double)(s.w - 1u) * (2.0 * RR_PI);
    const double psi = phi - RR_PI;
    const rr_sincos_t t = rr_sincos(theta);
    const rr_sincos_t p = rr_sincos(psi);
    out[0] = p.c * t.s, out[1] = t.c, out[2] = p.s * t.s;
}

// p_env(l): the solid-angle density of sky_sample's directions at l = (lx, ly, lz), which need not be a unit vector.
SKY_HD double sky_density(const SkyDev& s, double lx, double ly, double lz) {
    const double inv = 1.0 / rr_sqrt(lx * lx + ly * ly + lz * lz);  // Vector::unit: Div<f64> multiplies by the reciprocal
    const double dx = lx * inv, dy = ly * inv, dz = lz * inv;
    const double phi = rr_atan2(dz, dx) + RR_PI;  // Scene::background's, lib.rs:254-263
    const double theta = rr_acos(dy);
    const double wm1 = (double)(s.w - 1u), hm1 = (double)(s.h - 1u);
    const double x = phi / (2.0 * RR_PI) * wm1;
    const double y = theta / RR_PI * hm1;
    const uint32_t i = sky_cell_index(rr_floor(y), s.h - 2u);
    const uint32_t j = sky_cell_index(rr_floor(x), s.w - 2u);
    const double sn = rr_sqrt(1.0 - dy * dy);
    return ((sky_A(s, i)[j] / s.T) * (wm1 * hm1)) / (((2.0 * RR_PI) * RR_PI) * sn);
}

}  // namespace rayrs
