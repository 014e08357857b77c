// radiance_tree_device.h -- one diffuse bounce of include/rayrs_hip.h LIGHT TREE for radiance_tree.hip's kernels: MESH LIGHTS' bounce
// (radiance_mesh_device.h) with the group's arm drawn by the tree, descended from the shading point, and the met weight with the
// tree's probability of the triangle met.  p_R, the lamps' and the sky's arms, what a bounce hands the wave (MeshBounce) and the
// area-measure weights are MESH LIGHTS'; tree_sample, tree_probability and p_tri are radiance_tree_table.h's, the functions the
// host calls run.  All f64, unfused, in the header's operation order.
#pragma once
#include "device_path.h"
#include "radiance_mesh_device.h"
#include "radiance_tree_kernels.h"

namespace rayrs {

// The three draws b, u1, u2 are taken here.  A lane that drew the group descends the tree on its own: one 128-byte line a step,
// its fields read where they are used, then one 128-byte record.
template <bool SKY>
RR_DEV MeshBounce tree_bounce(V3 albedo, V3 thr, V3 position, V3 n, V3 l, Rng& rng, const LightsDev& lights, const TreeDev& tree,
                              const SkyDev& sky) {
    const uint32_t K = lights.n, M = K + 1u + (SKY ? 1u : 0u);
    const double m = (double)M;
    const double b = rng.next();
    const double u1 = rng.next();
    const double u2 = rng.next();
    uint32_t k = (uint32_t)(b * m);
    if (k > M - 1u) k = M - 1u;
    MeshBounce out;
    out.shadow = false;
    out.credit = mk(0.0, 0.0, 0.0);
    out.aim = MESH_NO_AIM;
    double p_tri = 0.0;
    if (k == K) {
        double q[3], ls[3], p_sel;
        const double pos[3] = {position.x, position.y, position.z};
        const uint32_t j = tree_sample(tree, pos, u1, u2, q, p_sel);
        const MeshTri* t = tree.tris + j;
        const double nj[3] = {t->n[0], t->n[1], t->n[2]};
        p_tri = tree_aim(pos, q, nj, t->A, p_sel, ls);
        out.l_s = mk(ls[0], ls[1], ls[2]);
        out.aim = t->slot;
    } else if (SKY && k == K + 1u) {
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
    const double ndl_s = v_dot(n, out.l_s);
    if (ndl_s > 0.0) {
        const double p_light = out.aim != MESH_NO_AIM ? p_tri / m : mesh_rest_density<SKY>(lights, sky, m, position, out.l_s);
        const double den = p_light + ndl_s * RR_FRAC_1_PI;
        if (den < (double)__builtin_inf()) {
            const V3 c = v_div(v_scale(v_scale(albedo, RR_FRAC_1_PI), ndl_s), den);
            out.credit = v_mul(thr, c);
            out.shadow = true;
        }
    }
    const double ndl = v_dot(n, l);
    out.pc = ndl * RR_FRAC_1_PI;
    const double pr = mesh_rest_density<SKY>(lights, sky, m, position, l);
    out.w_next = pr > 0.0 ? out.pc / (out.pc + pr) : 1.0;
    return out;
}

// The weight of the emission of entry j met by the path's ray Ray{o, d} at `position` = ray.point(t), where the triangle's normal
// is `normal` (either side): the cosine arm's pc against the group's density at that point, in solid angle, over M.
RR_DEV double tree_met_weight(const TreeDev& tree, uint32_t j, double m, double pc, V3 o, V3 d, V3 position, V3 normal) {
    const double x[3] = {o.x, o.y, o.z};
    const double p = (v_mag2(v_sub(o, position)) / (rr_fabs(v_dot(normal, d)) * tree.tris[j].A)) * tree_probability(tree, x, j);
    return p > 0.0 ? pc / (pc + p / m) : 1.0;
}

}  // namespace rayrs
