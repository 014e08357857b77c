// radiance_mesh_table.h -- a mesh-light group as a light (include/rayrs_hip.h MESH LIGHTS): the table's layout, mesh_sample and
// p_tri, written once for the host calls (rayrs_mesh_lights_sample, rayrs_mesh_lights_density: radiance_mesh_abi.cpp) and for
// radiance_mesh.hip's kernels.  All f64, unfused, in the header's operation order; the elementary functions are rayrs_numeric.h's.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/rayrs_numeric.h"
#include "radiance_sky_table.h"

namespace rayrs {

// One listed triangle, a 128-byte line: the host scene's f64 vertices, Triangle::new's unit normal and area, and the depth-first
// slot a walk answers with for it (Trav::best_prim).  path, depth and w are a light tree's (radiance_tree_table.h: the left/right
// word of the entry's leaf, bit k for depth k, the leaf's depth and the entry's power); a group without a tree leaves them 0.
struct MeshTri {
    double p1[3], p2[3], p3[3];
    double n[3];
    double A;
    uint32_t slot, path;
    uint32_t depth, pad0;
    double w;
};
static_assert(sizeof(MeshTri) == 128, "MeshTri");

// The group of N >= 1 listed triangles, BY VALUE in the kernel arguments: two device pointers and T.
//   table    P[N], the inclusive prefix of the areas in list order -- the thing the search reads --, padded to a whole number of
//            128-byte lines, then the N records
//   listed   one bit per depth-first primitive slot, set for the listed triangles: ceil(n_prims / 32) words
struct MeshDev {
    const double* table;
    const uint32_t* listed;
    double T;
    uint32_t n, pad;
};
SKY_HD size_t mesh_prefix_doubles(uint32_t n) { return ((size_t)n + 15u) & ~(size_t)15u; }
SKY_HD size_t mesh_table_bytes(uint32_t n) { return mesh_prefix_doubles(n) * sizeof(double) + (size_t)n * sizeof(MeshTri); }
SKY_HD const double* mesh_P(const MeshDev& m) { return m.table; }
SKY_HD const MeshTri* mesh_tri(const MeshDev& m, uint32_t j) {
    return reinterpret_cast<const MeshTri*>(m.table + mesh_prefix_doubles(m.n)) + j;
}
// Is the primitive in depth-first slot `prim` a listed triangle?  (prim below the scene's primitive count.)
SKY_HD bool mesh_listed(const MeshDev& m, uint32_t prim) { return ((m.listed[prim >> 5] >> (prim & 31u)) & 1u) != 0u; }

// Triangle::new's arithmetic (geometry.rs:341-353) on a record whose vertices are set: n = nrm.unit(), A = nrm.mag() / 2.0.
SKY_HD void mesh_tri_finish(MeshTri& t) {
    const double e1x = t.p2[0] - t.p1[0], e1y = t.p2[1] - t.p1[1], e1z = t.p2[2] - t.p1[2];
    const double e2x = t.p3[0] - t.p1[0], e2y = t.p3[1] - t.p1[1], e2z = t.p3[2] - t.p1[2];
    const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const double mag = rr_sqrt(nx * nx + ny * ny + nz * nz);
    const double inv = 1.0 / mag;  // Vector::unit: Div<f64> multiplies by the reciprocal
    t.n[0] = nx * inv, t.n[1] = ny * inv, t.n[2] = nz * inv;
    t.A = mag / 2.0;
}

// mesh_sample(u1, u2): the entry j (returned) and its point q.  One search over P, then one record.
SKY_HD uint32_t mesh_sample(const MeshDev& m, double u1, double u2, double* q) {
    const double* P = mesh_P(m);
    const double ty = u1 * m.T;
    const uint32_t j = sky_first_above(P, m.n, ty);
    const double below = j > 0u ? P[j - 1u] : 0.0;
    const MeshTri* t = mesh_tri(m, j);
    const double r = (ty - below) / t->A;
    const double su = rr_sqrt(r);
    const double b0 = 1.0 - su;
    const double b1 = su * (1.0 - u2);
    const double b2 = su * u2;
    for (int c = 0; c < 3; c++) q[c] = (t->p1[c] * b0 + t->p2[c] * b1) + t->p3[c] * b2;
    return j;
}

// A shadow sample aimed at q of a triangle of unit normal n, seen from `position`: l_s = (q - position).unit() into l_s[3], and
// p_tri = (position - q).mag2() / (|n . l_s| * T), the solid-angle density at `position` of mesh_sample's points at q.
SKY_HD double mesh_aim(const double* position, const double* q, const double* n, double T, double* l_s) {
    const double dx = q[0] - position[0], dy = q[1] - position[1], dz = q[2] - position[2];
    const double inv = 1.0 / rr_sqrt(dx * dx + dy * dy + dz * dz);
    l_s[0] = dx * inv, l_s[1] = dy * inv, l_s[2] = dz * inv;
    const double ex = position[0] - q[0], ey = position[1] - q[1], ez = position[2] - q[2];
    const double d2 = ex * ex + ey * ey + ez * ez;
    const double c = rr_fabs(n[0] * l_s[0] + n[1] * l_s[1] + n[2] * l_s[2]);
    return d2 / (c * T);
}

}  // namespace rayrs
