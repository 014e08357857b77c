// radiance_tree_device.h -- one diffuse bounce of include/rayrs_hip.h LIGHT TREE for radiance_tree.hip's kernels: MESH LIGHTS' bounce
// (radiance_mesh_device.h group_bounce, the one text) with the group's arm drawn by the tree, descended from the shading point,
// and the met weight with the tree's probability of the triangle met -- the TreeDev overloads of what the bounce and the wave
// (radiance_group_wave.h) ask of a group.  p_R, the lamps' and the sky's arms, what a bounce hands the wave (MeshBounce) and the
// area-measure weights are MESH LIGHTS'; tree_sample, tree_probability and p_tri are radiance_tree_table.h's, the functions the
// host calls run.  All f64, unfused, in the header's operation order.
#pragma once
#include "device_path.h"
#include "radiance_mesh_device.h"
#include "radiance_tree_kernels.h"

namespace rayrs {

// The group's arm of the bounce, drawn by the tree descended from pos: the direction ls to the point u1, u2 draw, its density
// p_tri, and the slot of the triangle drawn.  One 128-byte line a step, its fields read where they are used, then one 128-byte
// record.
RR_DEV uint32_t group_aim(const TreeDev& tree, const double pos[3], double u1, double u2, double ls[3], double& p_tri) {
    double q[3], p_sel;
    const uint32_t j = tree_sample(tree, pos, u1, u2, q, p_sel);
    const MeshTri* t = tree.tris + j;
    const double nj[3] = {t->n[0], t->n[1], t->n[2]};
    p_tri = tree_aim(pos, q, nj, t->A, p_sel, ls);
    return t->slot;
}

// What the wave learns of the primitive its path's ray met: the entry of a listed triangle, one word of the entry table.
RR_DEV uint32_t group_met(const TreeDev& tree, uint32_t prim) { return tree.entry[prim]; }
RR_DEV bool group_listed(const TreeDev&, uint32_t met) { return met != TREE_UNLISTED; }

// The weight of the emission of entry j met by the path's ray Ray{o, d} at `position` = ray.point(t), where the triangle's normal
// is `normal` (either side): the cosine arm's pc against the group's density at that point, in solid angle, over M.
RR_DEV double group_met_weight(const TreeDev& tree, uint32_t j, double m, double pc, V3 o, V3 d, V3 position, V3 normal) {
    const double x[3] = {o.x, o.y, o.z};
    const double p = (v_mag2(v_sub(o, position)) / (rr_fabs(v_dot(normal, d)) * tree.tris[j].A)) * tree_probability(tree, x, j);
    return p > 0.0 ? pc / (pc + p / m) : 1.0;
}

}  // namespace rayrs
