// radiance_lit_device.h -- Material::evaluate with Some(pdf) (include/rayrs_hip.h LIGHT SAMPLING) for radiance_lit.hip's kernel:
// the one-sample mix of a light list and the cosine lobe on a LambertianDiffuse surface and on Plastic's diffuse arm
// (material.rs:259-281, :567-593, :943-959, :1027-1034; geometry.rs:138-152, :284-299), every other material as device_path.h
// has it.  All f64, unfused, in the header's operation order.
#pragma once
#include "device_path.h"
#include "radiance_lit_kernels.h"

namespace rayrs {

// Hittable::sample on the draws u1 then u2: geometry.rs:288-299 (plane), :142-152 (sphere).
RR_DEV V3 light_sample(uint32_t kind, uint32_t axis, double v0, double v1, double v2, double v3, double v4, double u1, double u2) {
    if (kind == PRIM_PLANE) {
        const double u = u1 * (v1 - v0) + v0;
        const double v = u2 * (v3 - v2) + v2;
        const uint32_t ax = axis >> 1;
        return ax == 0 ? mk(v4, u, v) : (ax == 1 ? mk(u, v4, v) : mk(u, v, v4));
    }
    const double phi = 2.0 * RR_PI * u2;
    const rr_sincos_t sc_phi = rr_sincos(phi);
    const double r = rr_sqrt(u1 * (1.0 - u1));
    const double x = sc_phi.c * 2.0 * r;
    const double y = sc_phi.s * 2.0 * r;
    const double z = 1.0 - 2.0 * u1;
    return v_add(v_scale(mk(x, y, z), v4), mk(v1, v2, v3));  // * radius2.sqrt() + origin
}

// One crossing of a light's surface at parameter t of Ray{position, l}: the squared distance over the area's projection,
// |n_k . l| with the LIGHT's normal at the crossing.
RR_DEV double light_crossing(V3 position, V3 l, double t, V3 nk, double area) {
    const V3 pt = hit_position(position, l, t);
    return v_mag2(v_sub(position, pt)) / (rr_fabs(v_dot(nk, l)) * area);
}

// p_k(l): the solid-angle density at `position` of the directions light_sample makes -- every crossing in front counts.
RR_DEV double light_density(const LightDev& L, V3 position, V3 l) {
    double p = 0.0;
    if (L.kind == PRIM_PLANE) {
        double t;
        if (plane_intersect(L.axis, L.v[0], L.v[1], L.v[2], L.v[3], L.v[4], position, l, t) && t > 0.0) {
            const double s = (L.axis & 1u) ? -1.0 : 1.0;
            const uint32_t ax = L.axis >> 1;
            p = light_crossing(position, l, t, mk(ax == 0 ? s : 0.0, ax == 1 ? s : 0.0, ax == 2 ? s : 0.0), L.v[5]);
        }
    } else {
        const V3 c = mk(L.v[1], L.v[2], L.v[3]);
        const V3 odiff = v_sub(position, c);
        const double a = v_mag2(l);
        const double b = 2.0 * v_dot(l, odiff);
        const double cc = v_mag2(odiff) - L.v[0];
        const double desc = b * b - 4.0 * a * cc;
        if (desc > 0.0) {
            const double sq = rr_sqrt(desc);
            const double t1 = (-b - sq) / (2.0 * a);
            const double t2 = (-b + sq) / (2.0 * a);
            if (t1 > 0.0) p = p + light_crossing(position, l, t1, v_unit(v_sub(hit_position(position, l, t1), c)), L.v[5]);
            if (t2 > 0.0) p = p + light_crossing(position, l, t2, v_unit(v_sub(hit_position(position, l, t2), c)), L.v[5]);
        }
    }
    return p;
}

// LambertianDiffuse::scatter with Some(pdf).  The list is read with a wave-uniform index throughout (it lives in the kernel
// arguments: scalar loads); the lane's own light is picked out of it by comparison, never by a lane's index.
RR_DEV Scatter lit_lambertian_scatter(V3 color_in, V3 position, V3 n, Rng& rng, const LightsDev& lights) {
    const uint32_t K = lights.n;
    V3 l;
    const double a = rng.next();
    if (a < 0.5) {
        const double b = rng.next();
        uint32_t k = (uint32_t)(b * (double)K);
        if (k > K - 1u) k = K - 1u;
        const double u1 = rng.next();
        const double u2 = rng.next();
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
        l = v_unit(v_sub(q, position));
    } else {  // Pdf::Cosine.generate: lambertian_scatter's direction
        l = cosine_direction(n, rng);
    }
    const double ndl = v_dot(n, l);
    double pdf = (double)__builtin_inf();
    if (!(ndl < 0.0)) {
        double pl = 0.0;
        for (uint32_t j = 0; j < K; j++) {
            const double p = light_density(lights.light[j], position, l);
            pl = j == 0u ? p : pl + p;
        }
        pl = pl / (double)K;
        pdf = 0.5 * pl + 0.5 * (ndl * RR_FRAC_1_PI);
    }
    const V3 brdf = v_scale(color_in, RR_FRAC_1_PI);
    return Scatter{true, v_div(v_scale(brdf, ndl), pdf), l};
}

// Material::evaluate(position, normal, view, pdf): LambertianDiffuse and Plastic's diffuse arm take the mix, Plastic's
// Cook-Torrance arm (after Plastic's own Fresnel draw) and the seven other materials ignore it.  K = 0 is pdf = None.
RR_DEV Scatter lit_material_evaluate(const SurfaceDev* s, V3 position, V3 n, V3 v, Rng& rng, const LightsDev& lights) {
    int kind = s->kind;
    bool lit = lights.n != 0u && kind == RAYRS_MAT_LAMBERTIAN;
    bool by_fresnel = false;
    double fresnel = 1.0;
    if (lights.n != 0u && kind == RAYRS_MAT_PLASTIC) {  // material.rs:567-593
        fresnel = schlick_scalar(1.0, s->ior, n, v);
        if (rng.next() < fresnel) kind = RAYRS_MAT_COOK_TORRANCE, by_fresnel = true;  // ct_scatter on the surface's layer
        else lit = true;
    }
    if (lit) return lit_lambertian_scatter(mk(s->color[0], s->color[1], s->color[2]), position, n, rng, lights);
    Scatter ev = material_evaluate_kind(kind, s, n, v, rng);
    if (by_fresnel && ev.scatter) ev.color = v_div(ev.color, fresnel);
    return ev;
}

}  // namespace rayrs
