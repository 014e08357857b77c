// radiance_mesh_device.h -- one diffuse bounce of include/rayrs_hip.h MESH LIGHTS for radiance_mesh.hip's kernels: DIRECT LIGHTING's
// bounce (SKY: SKY SAMPLING's) with one more light, the mesh-light group, between the lamps and the sky.  The lamps' points and
// densities, the sky's and the material evaluation are taken as they are (radiance_lit_device.h, radiance_sky_table.h,
// radiance_direct_device.h); mesh_sample and p_tri are radiance_mesh_table.h's, the functions the host calls run.  No density
// here sums over the group: a group-drawn sample is weighted in area measure at the point it drew, and the continuation at the
// point it meets (radiance_group_wave.h).  All f64, unfused, in the header's operation order.
#pragma once
#include "device_path.h"
#include "radiance_direct_device.h"
#include "radiance_mesh_kernels.h"
#include "radiance_sky_device.h"

namespace rayrs {

constexpr uint32_t MESH_NO_AIM = 0xffffffffu;  // the shadow ray was aimed at a lamp or at the sky

// p_R(position, l): the lamps' densities in list order, then (SKY) p_env(l), over M -- the group's is not among them.  With K = 0
// and no sky there is no such light: 0.0.
template <bool SKY>
RR_DEV double mesh_rest_density(const LightsDev& lights, const SkyDev& sky, double m, V3 position, V3 l) {
    const uint32_t K = lights.n;
    if (!SKY && K == 0u) return 0.0;
    double pr = 0.0;
    for (uint32_t j = 0; j < K; j++) {
        const double p = light_density(lights.light[j], position, l);
        pr = j == 0u ? p : pr + p;
    }
    if (SKY) {
        const double pe = sky_density(sky, l.x, l.y, l.z);
        pr = K == 0u ? pe : pr + pe;
    }
    return pr / m;
}

// What a diffuse bounce at (position, normal) adds to the loop's turn: DirectBounce's members, the cosine arm's density of the
// continuation (which weights a listed triangle it meets), and the slot of the triangle a group-drawn shadow ray is aimed at.
struct MeshBounce {
    bool shadow;
    V3 l_s;
    V3 credit;  // throughput * C
    double w_next, pc;
    uint32_t aim;  // MESH_NO_AIM: a lamp or the sky was drawn
};
// The group's arm of the bounce, drawn by area: the direction ls from pos to the point u1, u2 draw, its density p_tri, and the
// slot of the triangle drawn.  One binary search of the prefix table over global memory, then one 128-byte record.
RR_DEV uint32_t group_aim(const MeshDev& mesh, const double pos[3], double u1, double u2, double ls[3], double& p_tri) {
    double q[3];
    const uint32_t j = mesh_sample(mesh, u1, u2, q);
    const MeshTri* t = mesh_tri(mesh, j);
    const double nj[3] = {t->n[0], t->n[1], t->n[2]};
    p_tri = mesh_aim(pos, q, nj, mesh.T, ls);
    return t->slot;
}

// The three draws b, u1, u2 are taken here.  A lane that drew the group asks the group's own group_aim (GROUP: MeshDev, or
// radiance_tree_device.h's TreeDev); a lane that drew the sky searches the sky's table; a lane that drew a lamp picks it out of
// the kernel arguments by comparison.
template <bool SKY, class GROUP>
RR_DEV MeshBounce group_bounce(V3 albedo, V3 thr, V3 position, V3 n, V3 l, Rng& rng, const LightsDev& lights, const GROUP& group,
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
        double ls[3];
        const double pos[3] = {position.x, position.y, position.z};
        out.aim = group_aim(group, pos, u1, u2, ls, p_tri);
        out.l_s = mk(ls[0], ls[1], ls[2]);
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

// What the wave learns of the primitive its path's ray met: whether it is one of the group's triangles, one bitmap word.
RR_DEV bool group_met(const MeshDev& mesh, uint32_t prim) { return mesh_listed(mesh, prim); }
RR_DEV bool group_listed(const MeshDev&, bool met) { return met; }

// The weight of a listed triangle's emission met by the path's ray Ray{o, d} at `position` = ray.point(t), where the triangle's
// normal is `normal` (either side): the cosine arm's pc against the group's density at that point, in solid angle, over M.
RR_DEV double group_met_weight(const MeshDev& mesh, bool, double m, double pc, V3 o, V3 d, V3 position, V3 normal) {
    const double p = v_mag2(v_sub(o, position)) / (rr_fabs(v_dot(normal, d)) * mesh.T);
    return p > 0.0 ? pc / (pc + p / m) : 1.0;
}

}  // namespace rayrs
