// radiance_sky_device.h -- one diffuse bounce of include/rayrs_hip.h SKY SAMPLING for radiance_sky.hip's kernel: DIRECT LIGHTING's
// bounce (radiance_direct_device.h, whose material evaluation, membership test and DirectBounce it takes as they are) with
// M = K + 1 lights, the sky last.  sky_sample and p_env are radiance_sky_table.h's, the functions the host calls run.  All f64,
// unfused, in the header's operation order.
#pragma once
#include "device_path.h"
#include "radiance_direct_device.h"
#include "radiance_sky_kernels.h"

namespace rayrs {

// p_M(position, l): the lamps' densities in list order, then p_env(l), over M.  With K = 0 p_env is assigned.
RR_DEV double sky_mix_density(const LightsDev& lights, const SkyDev& sky, V3 position, V3 l) {
    const uint32_t K = lights.n;
    double pm = 0.0;
    for (uint32_t j = 0; j < K; j++) {
        const double p = light_density(lights.light[j], position, l);
        pm = j == 0u ? p : pm + p;
    }
    const double pe = sky_density(sky, l.x, l.y, l.z);
    pm = K == 0u ? pe : pm + pe;
    return pm / (double)(K + 1u);
}

// What a diffuse bounce at (position, normal) adds to the loop's turn, K >= 0.  The three draws b, u1, u2 are taken here.  A lane
// that drew the sky searches the table on its own (two binary searches over global memory); a lane that drew a lamp picks it out
// of the kernel arguments by comparison, as the lamps' own direct_bounce does.
RR_DEV DirectBounce direct_bounce(V3 albedo, V3 thr, V3 position, V3 n, V3 l, Rng& rng, const LightsDev& lights, const SkyDev& sky) {
    const uint32_t K = lights.n, M = K + 1u;
    const double b = rng.next();
    const double u1 = rng.next();
    const double u2 = rng.next();
    uint32_t k = (uint32_t)(b * (double)M);
    if (k > M - 1u) k = M - 1u;
    DirectBounce out;
    if (k == K) {
        double d[3];
        sky_sample(sky, u1, u2, d);
        out.l_s = mk(d[0], d[1], d[2]);
    } else {
        uint32_t kind = 0u, axis = 0u;
        double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0, v4 = 0.0;
        for (uint32_t j = 0; j < K; j++) {
            const LightDev& L = lights.light[j];
            if (j == k) {  // (a sphere's radius sits where a plane's pos does)
                kind = L.kind, axis = L.axis;
                v0 = L.v[0], v1 = L.v[1], v2 = L.v[2], v3 = L.v[3], v4 = L.v[4];
            }
        }
        const V3 q = light_sample(kind, axis, v0, v1, v2, v3, v4, u1, u2);
        out.l_s = v_unit(v_sub(q, position));
    }
    out.shadow = false;
    out.credit = mk(0.0, 0.0, 0.0);
    const double ndl_s = v_dot(n, out.l_s);
    if (ndl_s > 0.0) {
        const double den = sky_mix_density(lights, sky, position, out.l_s) + ndl_s * RR_FRAC_1_PI;
        if (den < (double)__builtin_inf()) {
            const V3 c = v_div(v_scale(v_scale(albedo, RR_FRAC_1_PI), ndl_s), den);
            out.credit = v_mul(thr, c);
            out.shadow = true;
        }
    }
    const double ndl = v_dot(n, l);
    const double pc = ndl * RR_FRAC_1_PI;
    const double pm = sky_mix_density(lights, sky, position, l);
    out.w_next = pm > 0.0 ? pc / (pc + pm) : 1.0;
    return out;
}

}  // namespace rayrs
