// radiance_tree_table.h -- a mesh-light group whose triangles are chosen by a light tree (include/rayrs_hip.h LIGHT TREE): the
// device layout, one step of the descent, tree_sample, tree_probability and the group's p_tri, written once for the host calls
// (rayrs_mesh_lights_tree_sample, rayrs_mesh_lights_tree_probability, rayrs_mesh_lights_density: radiance_tree_abi.cpp) and for
// radiance_tree.hip's kernels.  The records are radiance_mesh_table.h's, with the path word, the depth and the power in what is
// padding there.  All f64, unfused, in the header's operation order; the elementary functions are rayrs_numeric.h's.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/rayrs_numeric.h"
#include "radiance_mesh_table.h"

namespace rayrs {

constexpr uint32_t TREE_LEAF = 0x80000000u;      // a child reference with this bit is the leaf of entry (ref & ~TREE_LEAF)
constexpr uint32_t TREE_UNLISTED = 0xffffffffu;  // TreeDev::entry of a primitive slot that is no listed triangle

// What a node keeps of one child: the middle of the box over its entries' vertices, the box's squared half diagonal, its power.
struct TreeChild {
    double m[3];
    double r2;
    double W;
};
// One interior node, a 128-byte line: both children, and where they are -- another line of `nodes`, or (TREE_LEAF) a record.
struct TreeNode {
    TreeChild left, right;
    uint32_t left_ref, right_ref;
    double pad[5];
};
static_assert(sizeof(TreeNode) == 128, "TreeNode");

// The group of N >= 1 listed triangles, BY VALUE in the kernel arguments.
//   nodes    the N - 1 interior nodes, in the preorder of the interior nodes alone
//   tris     the N records, in list order (MeshTri with path, depth and w set)
//   entry    one word per depth-first primitive slot: the entry of a listed triangle, TREE_UNLISTED for every other slot
// The root is line 0, or (N == 1) the leaf of entry 0.
struct TreeDev {
    const TreeNode* nodes;
    const MeshTri* tris;
    const uint32_t* entry;
    uint32_t n, pad;
};
SKY_HD uint32_t tree_root(const TreeDev& t) { return t.n > 1u ? 0u : TREE_LEAF; }

// I_c of a child seen from x: W_c > 0.0 ? W_c / rr_max(|x - m_c|^2, r2_c) : 0.0.  A NaN distance is ignored by rr_max.
SKY_HD double tree_importance(const TreeChild& c, const double* x) {
    const double W = c.W;
    if (!(W > 0.0)) return 0.0;
    const double dx = x[0] - c.m[0], dy = x[1] - c.m[1], dz = x[2] - c.m[2];
    return W / rr_max(dx * dx + dy * dy + dz * dz, c.r2);
}

// P_l of a node seen from x.
SKY_HD double tree_left_probability(const TreeNode& nd, const double* x) {
    const double il = tree_importance(nd.left, x);
    const double s = il + tree_importance(nd.right, x);
    if (s > 0.0 && s < (double)__builtin_inf()) return il / s;
    return nd.left.W / (nd.left.W + nd.right.W);
}

// tree_sample's descent: the entry (returned), with u and p as they are at its leaf.  Every step follows a reference the build
// wrote, one level down a tree of N leaves, whatever u, x and the probabilities are: a NaN comparison goes right.
SKY_HD uint32_t tree_descend(const TreeDev& t, const double* x, double& u, double& p) {
    uint32_t ref = tree_root(t);
    p = 1.0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang loop unroll(disable)
#endif
    while (!(ref & TREE_LEAF)) {
        const TreeNode& nd = t.nodes[ref];
        const double pl = tree_left_probability(nd, x);
        const double pr = 1.0 - pl;
        if (u < pl) {
            u = u / pl, p = p * pl;
            ref = nd.left_ref;
        } else {
            u = (u - pl) / pr, p = p * pr;
            ref = nd.right_ref;
        }
    }
    return ref & ~TREE_LEAF;
}

// tree_probability(x, j): the same descent steered by j's path word (bit k set: right at depth k), the same expressions in the
// same order, so the p tree_sample returned when it arrived at j.
SKY_HD double tree_probability(const TreeDev& t, const double* x, uint32_t j) {
    const uint32_t path = t.tris[j].path, depth = t.tris[j].depth;
    uint32_t ref = tree_root(t);
    double p = 1.0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang loop unroll(disable)
#endif
    for (uint32_t k = 0; k < depth; k++) {
        const TreeNode& nd = t.nodes[ref];
        const double pl = tree_left_probability(nd, x);
        const double pr = 1.0 - pl;
        if (((path >> k) & 1u) == 0u) {
            p = p * pl;
            ref = nd.left_ref;
        } else {
            p = p * pr;
            ref = nd.right_ref;
        }
    }
    return p;
}

// tree_sample(x, u1, u2): the entry j (returned), its point q and p_sel.
SKY_HD uint32_t tree_sample(const TreeDev& t, const double* x, double u1, double u2, double* q, double& p_sel) {
    double u = u1;
    const uint32_t j = tree_descend(t, x, u, p_sel);
    const MeshTri* tri = t.tris + j;
    const double r = rr_min(u, 1.0);
    const double su = rr_sqrt(r);
    const double b0 = 1.0 - su;
    const double b1 = su * (1.0 - u2);
    const double b2 = su * u2;
    for (int c = 0; c < 3; c++) q[c] = (tri->p1[c] * b0 + tri->p2[c] * b1) + tri->p3[c] * b2;
    return j;
}

// A shadow sample aimed at q of entry j (unit normal n, area A), chosen with p_sel, seen from `position`: l_s into l_s[3], and
// p_tri = ((position - q).mag2() / (|n . l_s| * A)) * p_sel.
SKY_HD double tree_aim(const double* position, const double* q, const double* n, double A, double p_sel, double* l_s) {
    const double dx = q[0] - position[0], dy = q[1] - position[1], dz = q[2] - position[2];
    const double inv = 1.0 / rr_sqrt(dx * dx + dy * dy + dz * dz);
    l_s[0] = dx * inv, l_s[1] = dy * inv, l_s[2] = dz * inv;
    const double ex = position[0] - q[0], ey = position[1] - q[1], ez = position[2] - q[2];
    const double d2 = ex * ex + ey * ey + ez * ez;
    const double c = rr_fabs(n[0] * l_s[0] + n[1] * l_s[1] + n[2] * l_s[2]);
    return (d2 / (c * A)) * p_sel;
}

}  // namespace rayrs
