// radiance_direct_device.h -- one diffuse bounce of include/rayrs_hip.h DIRECT LIGHTING for radiance_direct.hip's kernel: the
// unlit Material::evaluate with Plastic's arm told, the shadow sample towards a light of the list and its balance-heuristic
// coefficient, and the weight the continuation's own meeting with a listed object gets.  The lights' points and densities are
// radiance_lit_device.h's.  All f64, unfused, in the header's operation order.
#pragma once
#include "device_path.h"
#include "radiance_direct_kernels.h"
#include "radiance_lit_device.h"

namespace rayrs {

// Material::evaluate(position, normal, view, None), draw for draw device_path.h's material_evaluate; `diffuse`: the surface is
// LambertianDiffuse, or Plastic whose Fresnel draw chose the diffuse arm (radiance_lit_device.h lit_material_evaluate's test).
RR_DEV Scatter direct_material_evaluate(const SurfaceDev* s, V3 n, V3 v, Rng& rng, bool& diffuse) {
    int kind = s->kind;
    diffuse = kind == RAYRS_MAT_LAMBERTIAN;
    bool by_fresnel = false;
    double fresnel = 1.0;
    if (kind == RAYRS_MAT_PLASTIC) {  // material.rs:567-593
        fresnel = schlick_scalar(1.0, s->ior, n, v);
        if (rng.next() < fresnel) kind = RAYRS_MAT_COOK_TORRANCE, by_fresnel = true;
        else kind = RAYRS_MAT_LAMBERTIAN, diffuse = true;
    }
    Scatter ev = material_evaluate_kind(kind, s, n, v, rng);
    if (by_fresnel && ev.scatter) ev.color = v_div(ev.color, fresnel);
    return ev;
}

// p_L(position, l): the sum of the lights' densities in list order, over K.  The table is read with a wave-uniform index.
RR_DEV double direct_list_density(const LightsDev& lights, V3 position, V3 l) {
    const uint32_t K = lights.n;
    double pl = 0.0;
    for (uint32_t j = 0; j < K; j++) {
        const double p = light_density(lights.light[j], position, l);
        pl = j == 0u ? p : pl + p;
    }
    return pl / (double)K;
}

// Is the object in depth-first slot `prim` in the list (set membership)?  Wave-uniform reads, the lane's own by comparison.
RR_DEV bool direct_listed(const LightsDev& lights, const LightSlotsDev& slots, uint32_t prim) {
    bool in = false;
    for (uint32_t j = 0; j < lights.n; j++) in = in || slots.prim[j] == prim;
    return in;
}

// What the direct wave's kernels pass where the sky's are handed the sky: the lamps of the list are the only lights.
struct NoSky {};

// What a diffuse bounce at (position, normal) adds to the loop's turn, K >= 1.  The three draws b, u1, u2 are taken here.
struct DirectBounce {
    bool shadow;  // a shadow ray Ray{position, l_s} is to be traced, worth `credit` * emit() of a listed object it meets
    V3 l_s;
    V3 credit;    // throughput * C
    double w_next;
};
RR_DEV DirectBounce direct_bounce(V3 albedo, V3 thr, V3 position, V3 n, V3 l, Rng& rng, const LightsDev& lights, const NoSky&) {
    const uint32_t K = lights.n;
    const double b = rng.next();
    const double u1 = rng.next();
    const double u2 = rng.next();
    uint32_t k = (uint32_t)(b * (double)K);
    if (k > K - 1u) k = K - 1u;
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
    DirectBounce out;
    out.shadow = false;
    out.l_s = v_unit(v_sub(q, position));
    out.credit = mk(0.0, 0.0, 0.0);
    const double ndl_s = v_dot(n, out.l_s);
    if (ndl_s > 0.0) {
        const double den = direct_list_density(lights, position, out.l_s) + ndl_s * RR_FRAC_1_PI;
        if (den < (double)__builtin_inf()) {
            const V3 c = v_div(v_scale(v_scale(albedo, RR_FRAC_1_PI), ndl_s), den);
            out.credit = v_mul(thr, c);
            out.shadow = true;
        }
    }
    const double ndl = v_dot(n, l);
    const double pc = ndl * RR_FRAC_1_PI;
    const double pl = direct_list_density(lights, position, l);
    out.w_next = pl > 0.0 ? pc / (pc + pl) : 1.0;
    return out;
}

}  // namespace rayrs
