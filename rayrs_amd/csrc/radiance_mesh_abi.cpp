// radiance_mesh_abi.cpp -- the radiance queries with a mesh-light group among the lights of include/rayrs_hip.h (MESH LIGHTS): the
// handle, its table of the host scene's triangles, the device copy, the three host-only calls over radiance_mesh_table.h's
// functions, and the entry points.  The refusals, the light table, the launches and the host forms are the lit queries'
// (radiance_lit_abi.cpp), taken with LitCall::direct, LitCall::sky and LitCall::mesh set.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <memory>

#include "../../include/rayrs_hip.h"
#include "../../include/rayrs_numeric.h"
#include "radiance_lit_host.hpp"
#include "radiance_mesh_table.h"

// The device copy may still be read by the scene's last radiance launch: wait for the event lit_scratch_end recorded behind it,
// as the next user of the scratch would.
rayrs_mesh_lights::~rayrs_mesh_lights() {
    if (!uploaded || !scene || scene->device < 0) return;
    (void)hipSetDevice(scene->device);
    if (scene->queries.strip_in_use) (void)hipEventSynchronize(scene->queries.ev_done);
}

namespace rayrs {
namespace {

// The group's table on the host, as the kernels take it (`table` and `listed` are host pointers).
MeshDev mesh_host_table(const rayrs_mesh_lights* m) {
    MeshDev out;
    std::memset(&out, 0, sizeof(out));
    out.table = m->table.data(), out.listed = m->listed.data(), out.T = m->total, out.n = m->n;
    return out;
}

// The vertices of the triangle in depth-first slot p: the record's f32 widened (a compact scene's vertices are exactly
// representable in f32) or its f64, the values Triangle::new was given.
void triangle_vertices(const rayrs_scene* scene, uint32_t p, MeshTri& t) {
    const uint32_t* rec = prim_record(scene, p);
    double v[9];
    if (scene->flat.compact) {
        float f[9];
        std::memcpy(f, rec, sizeof(f));
        for (int k = 0; k < 9; k++) v[k] = (double)f[k];
    } else {
        std::memcpy(v, rec, sizeof(v));
    }
    for (int k = 0; k < 3; k++) t.p1[k] = v[k], t.p2[k] = v[3 + k], t.p3[k] = v[6 + k];
}

// The refusals of the calls' mesh arguments that are of the RAYRS_INVALID_ARG group whatever else is asked.
bool mesh_args_invalid(uint32_t sky) { return sky > 1u; }

}  // namespace

int mesh_device_table(const rayrs_mesh_lights* mesh, MeshDev* out) {
    rayrs_mesh_lights* m = const_cast<rayrs_mesh_lights*>(mesh);  // (the lazy upload is the handle's own business)
    if (!m->uploaded) {
        HIP_TRY(m->d_table.upload(m->table.data(), m->table.size() * sizeof(double)));
        HIP_TRY(m->d_listed.upload(m->listed.data(), m->listed.size() * sizeof(uint32_t)));
        m->uploaded = true;
    }
    MeshDev t = mesh_host_table(m);
    t.table = m->d_table.as<const double>(), t.listed = m->d_listed.as<const uint32_t>();
    *out = t;
    return RAYRS_OK;
}

// rayrs_mesh_lights_create past its null checks: the list's refusals in the header's order, then the handle with its table.
int mesh_lights_make(rayrs_scene* scene, const uint32_t* tris, uint64_t n_tris, std::unique_ptr<rayrs_mesh_lights>& m) {
    if (!tris && n_tris > 0u) return RAYRS_INVALID_ARG;
    const size_t n_objects = scene->flat.prim_object.size();
    std::vector<uint32_t> seen((n_objects + 31u) / 32u, 0u);  // over OBJECT indices: the duplicate check
    // (2^31 distinct indices below the object count would pass the loop only with as many objects; the size is refused first so
    // that the loop is bounded by the object count: a longer list has a duplicate or an index out of range within n_objects + 1)
    const uint64_t scan = n_tris < (uint64_t)n_objects + 1u ? n_tris : (uint64_t)n_objects + 1u;
    for (uint64_t k = 0; k < scan; k++) {
        const uint32_t t = tris[k];
        if (t >= n_objects) return RAYRS_INVALID_ARG;
        if ((seen[t >> 5] >> (t & 31u)) & 1u) return RAYRS_INVALID_ARG;
        seen[t >> 5] |= 1u << (t & 31u);
    }
    if (n_tris >= (1ull << 31)) return RAYRS_INVALID_ARG;
    const std::vector<uint32_t>& map = lit_object_prim(scene);
    for (uint64_t k = 0; k < n_tris; k++)
        if ((lit_prim_tag(scene, map[tris[k]]) & 3u) != PRIM_TRIANGLE) return RAYRS_UNSUPPORTED;
    for (uint64_t k = 0; k < n_tris; k++) {  // DIRECT LIGHTING's material rule (radiance_lit_abi.cpp direct_list_unsupported)
        const SurfaceDev& s = scene->surfaces[lit_prim_tag(scene, map[tris[k]]) >> 8];
        const bool dark = s.emit[0] == 0.0 && s.emit[1] == 0.0 && s.emit[2] == 0.0;
        const bool always_scatters = s.kind == RAYRS_MAT_LAMBERTIAN || s.kind == RAYRS_MAT_REFLECT || s.kind == RAYRS_MAT_GLASS;
        if (!dark && !always_scatters) return RAYRS_UNSUPPORTED;
    }
    m.reset(new rayrs_mesh_lights());
    m->scene = scene;
    m->n = (uint32_t)n_tris;
    if (m->n != 0u) {
        m->table.assign(mesh_table_bytes(m->n) / sizeof(double), 0.0);
        m->listed.assign((scene->flat.prim_object.size() + 31u) / 32u, 0u);
        double* P = m->table.data();
        MeshTri* rec = reinterpret_cast<MeshTri*>(m->table.data() + mesh_prefix_doubles(m->n));
        for (uint32_t j = 0; j < m->n; j++) {
            MeshTri& t = rec[j];
            t.slot = map[tris[j]];
            triangle_vertices(scene, t.slot, t);
            mesh_tri_finish(t);
            P[j] = j == 0u ? t.A : P[j - 1u] + t.A;
            m->listed[t.slot >> 5] |= 1u << (t.slot & 31u);
        }
        m->total = P[m->n - 1u];
        if (!(m->total > 0.0) || !std::isfinite(m->total)) return RAYRS_UNSUPPORTED;
    }
    return RAYRS_OK;
}

}  // namespace rayrs

using namespace rayrs;

extern "C" {

int rayrs_mesh_lights_create(rayrs_scene* scene, const uint32_t* tris, uint64_t n_tris, rayrs_mesh_lights** out) {
    RAYRS_GUARDED({
    if (!scene || !out) return RAYRS_INVALID_ARG;
    std::unique_ptr<rayrs_mesh_lights> m;
    RAYRS_TRY(mesh_lights_make(scene, tris, n_tris, m));
    *out = m.release();
    return RAYRS_OK;
    })
}

void rayrs_mesh_lights_destroy(rayrs_mesh_lights* mesh) { delete mesh; }

int rayrs_mesh_lights_table(const rayrs_mesh_lights* mesh, double* areas, double* total) {
    RAYRS_GUARDED({
    if (!mesh || (!areas && !total)) return RAYRS_INVALID_ARG;
    const MeshDev t = mesh_host_table(mesh);
    if (areas)
        for (uint32_t j = 0; j < t.n; j++) areas[j] = mesh_tri(t, j)->A;
    if (total) *total = t.T;
    return RAYRS_OK;
    })
}

int rayrs_mesh_lights_sample(const rayrs_mesh_lights* mesh, const double* u, uint64_t n, uint32_t* j, double* q) {
    RAYRS_GUARDED({
    if (!mesh || !u || !j || !q) return RAYRS_INVALID_ARG;
    if (mesh->n == 0u || mesh->tree) return RAYRS_UNSUPPORTED;  // (a tree's draw needs a position: rayrs_mesh_lights_tree_sample)
    const MeshDev t = mesh_host_table(mesh);
    for (uint64_t k = 0; k < n; k++) j[k] = mesh_sample(t, u[2u * k], u[2u * k + 1u], q + 3u * k);
    return RAYRS_OK;
    })
}

int rayrs_mesh_lights_density(const rayrs_mesh_lights* mesh, const double* position, const uint32_t* j, const double* q, uint64_t n,
                              double* p) {
    RAYRS_GUARDED({
    if (!mesh || !position || !j || !q || !p) return RAYRS_INVALID_ARG;
    for (uint64_t k = 0; k < n; k++)
        if (j[k] >= mesh->n) return RAYRS_INVALID_ARG;
    if (mesh->n == 0u) return RAYRS_UNSUPPORTED;
    if (mesh->tree) return tree_host_density(mesh, position, j, q, n, p);  // LIGHT TREE's p_tri
    const MeshDev t = mesh_host_table(mesh);
    for (uint64_t k = 0; k < n; k++) {
        double l_s[3];
        p[k] = mesh_aim(position + 3u * k, q + 3u * k, mesh_tri(t, j[k])->n, t.T, l_s);
    }
    return RAYRS_OK;
    })
}

int rayrs_scene_radiance_mesh(rayrs_scene* scene, const double* origin, const double* direction, uint64_t n, uint32_t samples,
                              uint32_t max_bounces, uint32_t sample_chunk, uint64_t seed, uint64_t index_base, uint32_t fast_traversal,
                              const uint32_t* lights, uint32_t n_lights, const rayrs_mesh_lights* mesh, uint32_t sky, double* radiance,
                              uint32_t* queries) {
    RAYRS_GUARDED({
    if (mesh_args_invalid(sky)) return RAYRS_INVALID_ARG;
    return lit_entry(scene, LitCall{LIT_START_RAY, samples, max_bounces, sample_chunk, 0.0, seed, index_base, fast_traversal, lights, n_lights, true, sky == 1u, mesh},
                     origin, direction, n, radiance, queries, false, nullptr);
    })
}

int rayrs_scene_radiance_mesh_launch(rayrs_scene* scene, const double* origin, const double* direction, uint64_t n, uint32_t samples,
                                     uint32_t max_bounces, uint32_t sample_chunk, uint64_t seed, uint64_t index_base,
                                     uint32_t fast_traversal, const uint32_t* lights, uint32_t n_lights, const rayrs_mesh_lights* mesh,
                                     uint32_t sky, double* radiance, uint32_t* queries, void* hip_stream) {
    RAYRS_GUARDED({
    if (mesh_args_invalid(sky)) return RAYRS_INVALID_ARG;
    return lit_entry(scene, LitCall{LIT_START_RAY, samples, max_bounces, sample_chunk, 0.0, seed, index_base, fast_traversal, lights, n_lights, true, sky == 1u, mesh},
                     origin, direction, n, radiance, queries, true, hip_stream);
    })
}

int rayrs_scene_irradiance_mesh(rayrs_scene* scene, const double* position, const double* normal, uint64_t n, uint32_t samples,
                                uint32_t max_bounces, uint32_t sample_chunk, double bias, uint64_t seed, uint64_t index_base,
                                uint32_t fast_traversal, const uint32_t* lights, uint32_t n_lights, const rayrs_mesh_lights* mesh,
                                uint32_t sky, double* radiance, uint32_t* queries) {
    RAYRS_GUARDED({
    if (mesh_args_invalid(sky)) return RAYRS_INVALID_ARG;
    return lit_entry(scene, LitCall{LIT_START_POINT, samples, max_bounces, sample_chunk, bias, seed, index_base, fast_traversal, lights, n_lights, true, sky == 1u, mesh},
                     position, normal, n, radiance, queries, false, nullptr);
    })
}

int rayrs_scene_irradiance_mesh_launch(rayrs_scene* scene, const double* position, const double* normal, uint64_t n, uint32_t samples,
                                       uint32_t max_bounces, uint32_t sample_chunk, double bias, uint64_t seed, uint64_t index_base,
                                       uint32_t fast_traversal, const uint32_t* lights, uint32_t n_lights, const rayrs_mesh_lights* mesh,
                                       uint32_t sky, double* radiance, uint32_t* queries, void* hip_stream) {
    RAYRS_GUARDED({
    if (mesh_args_invalid(sky)) return RAYRS_INVALID_ARG;
    return lit_entry(scene, LitCall{LIT_START_POINT, samples, max_bounces, sample_chunk, bias, seed, index_base, fast_traversal, lights, n_lights, true, sky == 1u, mesh},
                     position, normal, n, radiance, queries, true, hip_stream);
    })
}

int rayrs_render_mesh(rayrs_scene* scene, const rayrs_camera* camera, uint64_t seed, uint32_t samples, uint32_t max_bounces,
                      uint32_t sample_chunk, uint32_t fast_traversal, const uint32_t* lights, uint32_t n_lights,
                      const rayrs_mesh_lights* mesh, uint32_t sky, double* out_rgb, uint32_t* queries) {
    RAYRS_GUARDED({
    if (mesh_args_invalid(sky)) return RAYRS_INVALID_ARG;
    return lit_render(scene, camera, LitCall{LIT_START_PIXEL, samples, max_bounces, sample_chunk, 0.0, seed, 0u, fast_traversal, lights, n_lights, true, sky == 1u, mesh},
                      out_rgb, queries);
    })
}

}  // extern "C"
