// radiance_tree_abi.cpp -- a mesh-light group whose triangles are chosen by a light tree (include/rayrs_hip.h LIGHT TREE): the
// creator, which is rayrs_mesh_lights_create's (radiance_mesh_abi.cpp mesh_lights_make) with the powers' refusals and the build on
// top, the device copy, and the host-only calls over radiance_tree_table.h's functions.  The handle is the group's; the entry
// points that take it are MESH LIGHTS', which tell a tree handle by its kind (radiance_lit_abi.cpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>

#include "../../include/rayrs_hip.h"
#include "../../include/rayrs_numeric.h"
#include "radiance_lit_host.hpp"
#include "radiance_tree_table.h"

namespace rayrs {
namespace {

constexpr uint32_t NONE = 0xffffffffu;

MeshTri* tree_records(rayrs_mesh_lights* m) { return reinterpret_cast<MeshTri*>(m->table.data() + mesh_prefix_doubles(m->n)); }

// The group's tree on the host, as the kernels take it (host pointers).
TreeDev tree_host_table(const rayrs_mesh_lights* m) {
    TreeDev out;
    std::memset(&out, 0, sizeof(out));
    out.nodes = m->nodes.data(), out.tris = tree_records(const_cast<rayrs_mesh_lights*>(m)), out.entry = m->entry.data();
    out.n = m->n;
    return out;
}

// The header's build: top-down over a permutation of the entries, nodes numbered in preorder.
struct TreeBuild {
    rayrs_mesh_lights* m;
    MeshTri* rec;
    std::vector<uint32_t> perm;
    std::vector<double> key;  // c = (p1 + p2) + p3 of every entry: three per entry

    // The node over perm[lo .. hi): its reference (returned) and what its parent keeps of it.
    uint32_t node(uint32_t lo, uint32_t hi, uint32_t depth, uint32_t path, TreeChild& me) {
        const uint32_t pre = (uint32_t)m->pre_right.size();
        m->pre_right.push_back(NONE), m->pre_entry.push_back(NONE);
        m->pre_mrw.resize(m->pre_mrw.size() + 5u, 0.0);
        double blo[3], bhi[3];  // the box over the entries' vertices
        for (uint32_t i = lo; i < hi; i++) {
            const MeshTri& t = rec[perm[i]];
            const double* v[3] = {t.p1, t.p2, t.p3};
            for (int k = 0; k < 3; k++)
                for (int c = 0; c < 3; c++) {
                    const double x = v[k][c];
                    if (i == lo && k == 0) blo[c] = bhi[c] = x;
                    if (x < blo[c]) blo[c] = x;
                    if (x > bhi[c]) bhi[c] = x;
                }
        }
        for (int c = 0; c < 3; c++) me.m[c] = (blo[c] + bhi[c]) * 0.5;
        const double hx = bhi[0] - me.m[0], hy = bhi[1] - me.m[1], hz = bhi[2] - me.m[2];
        me.r2 = hx * hx + hy * hy + hz * hz;
        uint32_t ref;
        if (hi - lo == 1u) {
            const uint32_t j = perm[lo];
            rec[j].path = path, rec[j].depth = depth;
            me.W = rec[j].w;
            m->pre_entry[pre] = j;
            ref = TREE_LEAF | j;
        } else {
            double klo[3], khi[3];  // the bounds of the centroid keys
            for (uint32_t i = lo; i < hi; i++)
                for (int c = 0; c < 3; c++) {
                    const double x = key[3u * perm[i] + c];
                    if (i == lo) klo[c] = khi[c] = x;
                    if (x < klo[c]) klo[c] = x;
                    if (x > khi[c]) khi[c] = x;
                }
            int axis = 0;
            for (int c = 1; c < 3; c++)
                if (khi[c] - klo[c] > khi[axis] - klo[axis]) axis = c;
            std::sort(perm.begin() + lo, perm.begin() + hi, [&](uint32_t a, uint32_t b) {
                const double ka = key[3u * a + axis], kb = key[3u * b + axis];
                return ka < kb || (ka == kb && a < b);
            });
            const uint32_t mid = lo + (hi - lo + 1u) / 2u;
            const uint32_t line = (uint32_t)m->nodes.size();
            m->nodes.emplace_back();
            TreeNode nd;
            std::memset(&nd, 0, sizeof(nd));
            nd.left_ref = node(lo, mid, depth + 1u, path, nd.left);
            m->pre_right[pre] = (uint32_t)m->pre_right.size();
            nd.right_ref = node(mid, hi, depth + 1u, path | (1u << depth), nd.right);
            m->nodes[line] = nd;
            me.W = nd.left.W + nd.right.W;
            ref = line;
        }
        double* out = m->pre_mrw.data() + 5u * pre;
        out[0] = me.m[0], out[1] = me.m[1], out[2] = me.m[2], out[3] = me.r2, out[4] = me.W;
        return ref;
    }
};

}  // namespace

int tree_device_table(const rayrs_mesh_lights* mesh, TreeDev* out) {
    rayrs_mesh_lights* m = const_cast<rayrs_mesh_lights*>(mesh);  // (the lazy upload is the handle's own business)
    if (!m->uploaded) {
        HIP_TRY(m->d_table.upload(m->table.data(), m->table.size() * sizeof(double)));
        // (N == 1 has no interior node: one line of zeros, so that the pointer is one)
        const TreeNode none{};
        HIP_TRY(m->d_nodes.upload(m->nodes.empty() ? &none : m->nodes.data(), (m->nodes.empty() ? 1u : m->nodes.size()) * sizeof(TreeNode)));
        HIP_TRY(m->d_entry.upload(m->entry.data(), m->entry.size() * sizeof(uint32_t)));
        m->uploaded = true;
    }
    TreeDev t = tree_host_table(m);
    t.nodes = m->d_nodes.as<const TreeNode>();
    t.tris = reinterpret_cast<const MeshTri*>(m->d_table.as<const double>() + mesh_prefix_doubles(m->n));
    t.entry = m->d_entry.as<const uint32_t>();
    *out = t;
    return RAYRS_OK;
}

int tree_host_density(const rayrs_mesh_lights* mesh, const double* position, const uint32_t* j, const double* q, uint64_t n, double* p) {
    const TreeDev t = tree_host_table(mesh);
    for (uint64_t k = 0; k < n; k++) {
        const MeshTri* tri = t.tris + j[k];
        double l_s[3];
        p[k] = tree_aim(position + 3u * k, q + 3u * k, tri->n, tri->A, tree_probability(t, position + 3u * k, j[k]), l_s);
    }
    return RAYRS_OK;
}

}  // namespace rayrs

using namespace rayrs;

extern "C" {

int rayrs_mesh_lights_create_tree(rayrs_scene* scene, const uint32_t* tris, uint64_t n_tris, rayrs_mesh_lights** out) {
    RAYRS_GUARDED({
    if (!scene || !out) return RAYRS_INVALID_ARG;
    std::unique_ptr<rayrs_mesh_lights> m;
    RAYRS_TRY(mesh_lights_make(scene, tris, n_tris, m));
    m->tree = true;
    m->listed.clear();
    if (m->n != 0u) {
        TreeBuild b{m.get(), tree_records(m.get()), {}, {}};
        b.perm.resize(m->n), b.key.resize(3u * (size_t)m->n);
        for (uint32_t j = 0; j < m->n; j++) {
            MeshTri& t = b.rec[j];
            const double* e = scene->surfaces[lit_prim_tag(scene, t.slot) >> 8].emit;
            for (int c = 0; c < 3; c++)
                if (!(e[c] >= 0.0) || !std::isfinite(e[c])) return RAYRS_UNSUPPORTED;
            for (int c = 0; c < 3; c++)
                if (!std::isfinite(t.p1[c]) || !std::isfinite(t.p2[c]) || !std::isfinite(t.p3[c])) return RAYRS_UNSUPPORTED;
            t.w = t.A * ((e[0] + e[1]) + e[2]);
            for (int c = 0; c < 3; c++) b.key[3u * j + c] = (t.p1[c] + t.p2[c]) + t.p3[c];
            b.perm[j] = j;
        }
        m->nodes.reserve(m->n - 1u);
        TreeChild root;
        (void)b.node(0u, m->n, 0u, 0u, root);
        if (!(root.W > 0.0) || !std::isfinite(root.W)) return RAYRS_UNSUPPORTED;
        m->entry.assign(scene->flat.prim_object.size(), TREE_UNLISTED);
        for (uint32_t j = 0; j < m->n; j++) m->entry[b.rec[j].slot] = j;
    }
    *out = m.release();
    return RAYRS_OK;
    })
}

int rayrs_mesh_lights_tree_nodes(const rayrs_mesh_lights* mesh, double* mrw, uint32_t* right, uint32_t* entry) {
    RAYRS_GUARDED({
    if (!mesh || (!mrw && !right && !entry)) return RAYRS_INVALID_ARG;
    if (!mesh->tree) return RAYRS_UNSUPPORTED;
    if (mrw) std::copy(mesh->pre_mrw.begin(), mesh->pre_mrw.end(), mrw);
    if (right) std::copy(mesh->pre_right.begin(), mesh->pre_right.end(), right);
    if (entry) std::copy(mesh->pre_entry.begin(), mesh->pre_entry.end(), entry);
    return RAYRS_OK;
    })
}

int rayrs_mesh_lights_tree_entries(const rayrs_mesh_lights* mesh, double* power, uint32_t* path, uint32_t* depth) {
    RAYRS_GUARDED({
    if (!mesh || (!power && !path && !depth)) return RAYRS_INVALID_ARG;
    if (!mesh->tree) return RAYRS_UNSUPPORTED;
    const TreeDev t = tree_host_table(mesh);
    for (uint32_t j = 0; j < mesh->n; j++) {
        if (power) power[j] = t.tris[j].w;
        if (path) path[j] = t.tris[j].path;
        if (depth) depth[j] = t.tris[j].depth;
    }
    return RAYRS_OK;
    })
}

int rayrs_mesh_lights_tree_sample(const rayrs_mesh_lights* mesh, const double* position, const double* u, uint64_t n, uint32_t* j,
                                  double* q, double* p_sel) {
    RAYRS_GUARDED({
    if (!mesh || !position || !u || !j || !q || !p_sel) return RAYRS_INVALID_ARG;
    if (!mesh->tree || mesh->n == 0u) return RAYRS_UNSUPPORTED;
    const TreeDev t = tree_host_table(mesh);
    for (uint64_t k = 0; k < n; k++) j[k] = tree_sample(t, position + 3u * k, u[2u * k], u[2u * k + 1u], q + 3u * k, p_sel[k]);
    return RAYRS_OK;
    })
}

int rayrs_mesh_lights_tree_probability(const rayrs_mesh_lights* mesh, const double* position, const uint32_t* j, uint64_t n, double* p) {
    RAYRS_GUARDED({
    if (!mesh || !position || !j || !p) return RAYRS_INVALID_ARG;
    for (uint64_t k = 0; k < n; k++)
        if (j[k] >= mesh->n) return RAYRS_INVALID_ARG;
    if (!mesh->tree || mesh->n == 0u) return RAYRS_UNSUPPORTED;
    const TreeDev t = tree_host_table(mesh);
    for (uint64_t k = 0; k < n; k++) p[k] = tree_probability(t, position + 3u * k, j[k]);
    return RAYRS_OK;
    })
}

}  // extern "C"
