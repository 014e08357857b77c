// radiance_probe_table.h -- SH probes (include/rayrs_hip.h SH PROBES): a sample's direction from its two draws and the nine real
// harmonics of a direction, written once for the host calls (rayrs_probe_directions, rayrs_sh_basis: radiance_probe_abi.cpp),
// for the sample's start (radiance_wave_parts.h sample_start) and for the projection (radiance_probe.hip).  All f64, unfused, in
// the header's operation order; the elementary functions are rayrs_numeric.h's.
#pragma once
#include <stdint.h>

#include "../../include/rayrs_numeric.h"

#if defined(__HIPCC__)
#define PROBE_HD __host__ __device__ static inline
#else
#define PROBE_HD static inline
#endif

namespace rayrs {

// The f64 nearest to sqrt(1/4pi), sqrt(3/4pi), sqrt(15/4pi), sqrt(5/16pi), sqrt(15/16pi).
constexpr double SH_K0 = 0.28209479177387814;
constexpr double SH_K1 = 0.4886025119029199;
constexpr double SH_K2 = 1.0925484305920792;
constexpr double SH_K3 = 0.31539156525252005;
constexpr double SH_K4 = 0.5462742152960396;
constexpr uint32_t SH_COEFFS = 9;

// Sphere::sample (geometry.rs:142-152) on the unit sphere at the origin, on the draws u1 then u2: radiance_lit_device.h
// light_sample's sphere arm without the radius and the centre.  Not normalised again.
PROBE_HD void probe_direction(double u1, double u2, double* w) {
    const double phi = 2.0 * RR_PI * u2;
    const rr_sincos_t sc_phi = rr_sincos(phi);
    const double r = rr_sqrt(u1 * (1.0 - u1));
    w[0] = sc_phi.c * 2.0 * r;
    w[1] = sc_phi.s * 2.0 * r;
    w[2] = 1.0 - 2.0 * u1;
}

// The direction of sample s of probe i of a call: draws 0 and 1 of RADIANCE QUERY's key.
PROBE_HD void probe_sample_direction(uint64_t seed, uint64_t index, uint32_t s, double* w) {
    const uint64_t key = rr_path_key(seed, index, (uint64_t)s);
    const double u1 = rr_uniform(key, 0u);
    const double u2 = rr_uniform(key, 1u);
    probe_direction(u1, u2, w);
}

// Y_0 .. Y_8 on the components of (x, y, z) as they stand, every product from left to right.
PROBE_HD void sh_basis(double x, double y, double z, double* Y) {
    Y[0] = SH_K0;
    Y[1] = SH_K1 * y;
    Y[2] = SH_K1 * z;
    Y[3] = SH_K1 * x;
    Y[4] = (SH_K2 * x) * y;
    Y[5] = (SH_K2 * y) * z;
    Y[6] = SH_K3 * ((3.0 * z) * z - 1.0);
    Y[7] = (SH_K2 * x) * z;
    Y[8] = SH_K4 * (x * x - y * y);
}

}  // namespace rayrs
