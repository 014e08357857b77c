// abi.cpp -- the extern "C" boundary declared in include/rayrs_hip.h: each entry point is its argument checks and a call.
// A scene on its device is scene_device.cpp, a frame's plan frame_plan.cpp, a render render.cpp; the device self tests of
// rayrs_selftest.h are in selftest.cpp.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/rayrs_hip.h"
#include "rayrs_lab.h"
#include "scene_host.hpp"
#include "scene_internal.hpp"

using namespace rayrs;

namespace {
thread_local std::string g_last_error;
}  // namespace

namespace rayrs {
void set_last_error(const std::string& text) { g_last_error = text; }
int hip_fail(hipError_t e, const char* what) {
    g_last_error = std::string(what) + ": " + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? RAYRS_OOM : RAYRS_HIP_ERROR;
}
}  // namespace rayrs

static void push_triangle(ObjectList& l, Vec3 p1, Vec3 p2, Vec3 p3, uint32_t surf) {
    Object o;
    std::memset(&o, 0, sizeof(o));
    o.geom.kind = PRIM_TRIANGLE;
    o.geom.p1 = p1, o.geom.p2 = p2, o.geom.p3 = p3;
    o.surface = surf;
    l.objs.push_back(o);
}

template <typename T>
static int from_triangles(rayrs_objects* objs, const T* verts, uint32_t nverts, const uint32_t* idx, uint32_t ntris,
                          const rayrs_material* mat, const rayrs_emission* emission) {
    if (!objs || (!verts && nverts) || (!idx && ntris)) return RAYRS_INVALID_ARG;
    for (size_t i = 0; i < (size_t)ntris * 3; i++)
        if (idx[i] >= nverts) return RAYRS_INVALID_ARG;
    const int surf = objs->list.add_surface(mat, emission);
    if (surf < 0) return surf;
    objs->list.objs.reserve(objs->list.objs.size() + ntris);
    for (uint32_t t = 0; t < ntris; t++) {
        const T* a = verts + 3 * (size_t)idx[3 * t];
        const T* b = verts + 3 * (size_t)idx[3 * t + 1];
        const T* c = verts + 3 * (size_t)idx[3 * t + 2];
        push_triangle(objs->list, {(double)a[0], (double)a[1], (double)a[2]},
                      {(double)b[0], (double)b[1], (double)b[2]}, {(double)c[0], (double)c[1], (double)c[2]},
                      (uint32_t)surf);
    }
    return RAYRS_OK;
}

extern "C" {

const char* rayrs_strerror(int status) {
    switch (status) {
        case RAYRS_OK: return "ok";
        case RAYRS_INVALID_ARG: return "invalid argument (a reference assert! would have fired)";
        case RAYRS_HIP_ERROR: return "HIP runtime error";
        case RAYRS_OOM: return "out of memory";
        case RAYRS_NO_DEVICE: return "no HIP device for this scene";
        case RAYRS_UNSUPPORTED: return "unsupported (size or depth limit)";
        case RAYRS_IO_ERROR: return "file missing or malformed";
        case RAYRS_RCCL_ERROR: return "RCCL unavailable or failed";
        default: return "unknown status";
    }
}

const char* rayrs_last_error(void) { return g_last_error.c_str(); }

// ------------------------------------------------------------- Vec<Object>

int rayrs_objects_create(rayrs_objects** out) {
    RAYRS_GUARDED({
    if (!out) return RAYRS_INVALID_ARG;
    *out = new (std::nothrow) rayrs_objects();
    return *out ? RAYRS_OK : RAYRS_OOM;
    })
}

void rayrs_objects_destroy(rayrs_objects* objs) { delete objs; }

uint64_t rayrs_objects_len(const rayrs_objects* objs) { return objs ? objs->list.objs.size() : 0; }

int rayrs_object_sphere(rayrs_objects* objs, double radius, const double origin[3], const rayrs_material* mat,
                        const rayrs_emission* emission) {
    RAYRS_GUARDED({
    if (!objs || !origin) return RAYRS_INVALID_ARG;
    if (!(radius > 0.)) return RAYRS_INVALID_ARG;  // geometry.rs:97
    const int surf = objs->list.add_surface(mat, emission);
    if (surf < 0) return surf;
    Object o;
    std::memset(&o, 0, sizeof(o));
    o.geom.kind = PRIM_SPHERE;
    o.geom.radius2 = radius * radius;  // geometry.rs:99
    o.geom.origin = {origin[0], origin[1], origin[2]};
    o.surface = (uint32_t)surf;
    objs->list.objs.push_back(o);
    return RAYRS_OK;
    })
}

int rayrs_object_plane(rayrs_objects* objs, int axis, double umin, double umax, double vmin, double vmax, double pos,
                       const rayrs_material* mat, const rayrs_emission* emission) {
    RAYRS_GUARDED({
    if (!objs) return RAYRS_INVALID_ARG;
    if (!(umin < umax && vmin < vmax)) return RAYRS_INVALID_ARG;  // geometry.rs:205-212
    if (axis < 0 || axis > 5) return RAYRS_INVALID_ARG;
    const int surf = objs->list.add_surface(mat, emission);
    if (surf < 0) return surf;
    Object o;
    std::memset(&o, 0, sizeof(o));
    o.geom.kind = PRIM_PLANE;
    o.geom.axis = (uint32_t)axis;
    o.geom.u0 = umin, o.geom.u1 = umax, o.geom.v0 = vmin, o.geom.v1 = vmax, o.geom.pos = pos;
    o.surface = (uint32_t)surf;
    objs->list.objs.push_back(o);
    return RAYRS_OK;
    })
}

int rayrs_object_triangle(rayrs_objects* objs, const double p1[3], const double p2[3], const double p3[3],
                          const rayrs_material* mat, const rayrs_emission* emission) {
    RAYRS_GUARDED({
    if (!objs || !p1 || !p2 || !p3) return RAYRS_INVALID_ARG;
    const int surf = objs->list.add_surface(mat, emission);
    if (surf < 0) return surf;
    push_triangle(objs->list, {p1[0], p1[1], p1[2]}, {p2[0], p2[1], p2[2]}, {p3[0], p3[1], p3[2]}, (uint32_t)surf);
    return RAYRS_OK;
    })
}

int rayrs_object_from_triangles_f32(rayrs_objects* objs, const float* verts, uint32_t nverts, const uint32_t* idx,
                                    uint32_t ntris, const rayrs_material* mat, const rayrs_emission* emission) {
    RAYRS_GUARDED({
    return from_triangles<float>(objs, verts, nverts, idx, ntris, mat, emission);
    })
}

int rayrs_object_from_triangles_f64(rayrs_objects* objs, const double* verts, uint32_t nverts, const uint32_t* idx,
                                    uint32_t ntris, const rayrs_material* mat, const rayrs_emission* emission) {
    RAYRS_GUARDED({
    return from_triangles<double>(objs, verts, nverts, idx, ntris, mat, emission);
    })
}

int rayrs_object_from_spheres(rayrs_objects* objs, double radius, const double* centers, uint32_t n,
                              const rayrs_material* mat, const rayrs_emission* emission) {
    if (!objs || (!centers && n)) return RAYRS_INVALID_ARG;
    for (uint32_t i = 0; i < n; i++) RAYRS_TRY(rayrs_object_sphere(objs, radius, centers + 3 * (size_t)i, mat, emission));
    return RAYRS_OK;
}

int rayrs_object_box_geom(rayrs_objects* objs, const double ll[3], const double ur[3], const rayrs_material* mat,
                          const rayrs_emission* emission) {
    if (!objs || !ll || !ur) return RAYRS_INVALID_ARG;
    // lib.rs:444-505, same order (note: both Y faces sit at lower_left.y, as in the reference)
    const struct {
        int axis;
        double u0, u1, v0, v1, pos;
    } faces[6] = {
        {RAYRS_AXIS_X, ll[1], ur[1], ll[2], ur[2], ll[0]},    {RAYRS_AXIS_XREV, ll[1], ur[1], ll[2], ur[2], ur[0]},
        {RAYRS_AXIS_ZREV, ll[0], ur[0], ll[1], ur[1], ll[2]}, {RAYRS_AXIS_Z, ll[0], ur[0], ll[1], ur[1], ur[2]},
        {RAYRS_AXIS_YREV, ll[0], ur[0], ll[2], ur[2], ll[1]}, {RAYRS_AXIS_Y, ll[0], ur[0], ll[2], ur[2], ll[1]},
    };
    for (const auto& f : faces) RAYRS_TRY(rayrs_object_plane(objs, f.axis, f.u0, f.u1, f.v0, f.v1, f.pos, mat, emission));
    return RAYRS_OK;
}

// ------------------------------------------------------------------- Scene

void rayrs_scene_destroy(rayrs_scene* scene) { delete scene; }

int rayrs_scene_new(const rayrs_objects* objs, double z_near, double z_far, int heuristic, uint32_t splits,
                    uint32_t hdri_w, uint32_t hdri_h, const float* hdri_rgb, int device, rayrs_scene** out) {
    RAYRS_GUARDED({
    if (!objs || !out) return RAYRS_INVALID_ARG;
    *out = nullptr;
    std::unique_ptr<rayrs_scene> s(new rayrs_scene());
    RAYRS_TRY(build_flat_scene(objs->list, z_near, z_far, heuristic, splits, hdri_w, hdri_h, hdri_rgb, &s->flat));
    // Every traversal lane gets a stack of WalkTree::stack_need entries (12 in LDS, the rest in HBM: 1.3 MB per entry on a
    // 256-CU device).  The reference recurses as deep as its tree; a tree that needs more than 4096 pending
    // entries (a chain of thousands of nested objects) is refused instead of allocating gigabytes for it.
    if (std::max(s->flat.walk.stack_need, s->flat.gate.stack_need) > 4096u) {
        g_last_error = "walk tree needs " + std::to_string(std::max(s->flat.walk.stack_need, s->flat.gate.stack_need)) + " stack entries (limit 4096)";
        return RAYRS_UNSUPPORTED;
    }
    s->surfaces = objs->list.surfaces;
    s->n_objects = objs->list.objs.size();
    s->device = device;
    scene_configure_local(s.get());
    if (device >= 0) RAYRS_TRY(scene_upload(s.get()));
    *out = s.release();
    return RAYRS_OK;
    })
}

int rayrs_scene_info(const rayrs_scene* scene, rayrs_scene_info_t* info) {
    if (!scene || !info) return RAYRS_INVALID_ARG;
    const FlatScene& f = scene->flat;
    std::memset(info, 0, sizeof(*info));
    info->n_objects = scene->n_objects;
    info->n_interior = f.n_interior();
    info->n_prims = f.n_prims();
    info->root_ref = f.root_ref;
    info->depth = f.depth;
    info->compact = f.compact ? 1u : 0u;
    info->n_surfaces = (uint32_t)scene->surfaces.size();
    info->node_bytes = f.compact ? (uint32_t)sizeof(Node4F32) : (uint32_t)sizeof(Node4F64);
    info->n_wide = f.walk.n();
    info->wide_root_ref = f.walk.root_ref;
    info->wide_depth = f.walk.depth;
    info->gate_n_wide = f.gate.n();
    info->gate_root_ref = f.gate.root_ref;
    info->gate_depth = f.gate.depth;
    if (f.has_hot) {
        info->hot_n_wide = f.gate_hot.n();
        info->hot_root_ref = f.gate_hot.root_ref;
        info->hot_depth = f.gate_hot.depth;
        info->hot_first = f.hot.first;
        info->hot_count = f.hot.count;
        for (int i = 0; i < 6; i++) info->hot_box[i] = f.hot.box[i];
    }
    info->local_pool = (scene->local_ok && scene->tuning.local_pool != 1u) ? 1u : 0u;
    info->prim_bytes = 4u * (f.compact ? PRIM_DWORDS_COMPACT : PRIM_DWORDS_FULL);
    info->device_bytes = scene->device_bytes;
    for (int i = 0; i < 6; i++) info->root_box[i] = f.root_box[i];
    info->build_seconds = f.build_seconds;
    return RAYRS_OK;
}

int rayrs_scene_export_bvh(const rayrs_scene* scene, double* child_box, uint32_t* child_ref, uint32_t* prim_object) {
    if (!scene) return RAYRS_INVALID_ARG;
    const FlatScene& f = scene->flat;
    if (child_box && !f.child_box.empty()) std::memcpy(child_box, f.child_box.data(), f.child_box.size() * 8);
    if (child_ref && !f.child_ref.empty()) std::memcpy(child_ref, f.child_ref.data(), f.child_ref.size() * 4);
    if (prim_object && !f.prim_object.empty())
        std::memcpy(prim_object, f.prim_object.data(), f.prim_object.size() * 4);
    return RAYRS_OK;
}

static int export_tree(const WalkTree& t, double* wide_box, uint32_t* wide_ref) {
    if (wide_box && !t.box.empty()) std::memcpy(wide_box, t.box.data(), t.box.size() * 8);
    if (wide_ref && !t.ref.empty()) std::memcpy(wide_ref, t.ref.data(), t.ref.size() * 4);
    return RAYRS_OK;
}

int rayrs_scene_export_wide(const rayrs_scene* scene, double* wide_box, uint32_t* wide_ref) {
    return scene ? export_tree(scene->flat.walk, wide_box, wide_ref) : RAYRS_INVALID_ARG;
}

int rayrs_scene_export_gate_tree(const rayrs_scene* scene, double* wide_box, uint32_t* wide_ref) {
    return scene ? export_tree(scene->flat.gate, wide_box, wide_ref) : RAYRS_INVALID_ARG;
}

int rayrs_scene_export_hot_tree(const rayrs_scene* scene, double* wide_box, uint32_t* wide_ref) {
    return scene && scene->flat.has_hot ? export_tree(scene->flat.gate_hot, wide_box, wide_ref) : RAYRS_INVALID_ARG;
}

int rayrs_scene_clone_to_device(const rayrs_scene* scene, int device, rayrs_scene** out) {
    RAYRS_GUARDED({
        if (!scene || !out || device < 0) return RAYRS_INVALID_ARG;
        *out = nullptr;
        std::unique_ptr<rayrs_scene> s(new rayrs_scene());
        s->flat = scene->flat;
        s->surfaces = scene->surfaces;
        s->n_objects = scene->n_objects;
        s->tuning = scene->tuning;
        s->lab = scene->lab;
        s->device = device;
        scene_configure_local(s.get());
        RAYRS_TRY(scene_upload(s.get()));
        *out = s.release();
        return RAYRS_OK;
    })
}

int rayrs_scene_device(const rayrs_scene* scene) { return scene ? scene->device : -1; }

static int scene_quiesce(rayrs_scene* scene) {  // settings change between renders, never under one
    return scene->device >= 0 ? scene_settle(scene) : RAYRS_OK;
}

int rayrs_scene_set_tuning(rayrs_scene* scene, const rayrs_tuning* tuning) {
    if (!scene || !tuning) return RAYRS_INVALID_ARG;
    if (tuning->local_pool > 1u) return RAYRS_INVALID_ARG;
    RAYRS_TRY(scene_quiesce(scene));
    scene->tuning = *tuning;
    return RAYRS_OK;
}

#ifdef RAYRS_LAB_TICKS
// development build only (make LAB=1): the tick counters of the last render
extern "C" int rayrs_lab_ticks(rayrs_scene* scene, uint64_t out[16]) {
    if (!scene || !out || scene->device < 0) return RAYRS_INVALID_ARG;
    HIP_TRY(hipSetDevice(scene->device));
    Counters c;
    HIP_TRY(scene->frame.d_counters.download(&c, sizeof(c)));
    for (int i = 0; i < 16; i++) out[i] = c.lab_ticks[i];
    return RAYRS_OK;
}
#endif

// rayrs_lab.h: the kernels' development knobs (tests/ and scripts/ubench/ only)
int rayrs_lab_set(rayrs_scene* scene, const rayrs_lab_tuning* lab) {
    if (!scene || !lab) return RAYRS_INVALID_ARG;
    if (lab->stack_lds > 64u) return RAYRS_INVALID_ARG;  // 4 x 64 lanes x 65 entries x 4 B: what a workgroup's LDS can spare
    if (lab->hot_group != 0u && lab->hot_group != 0xffffffffu) return RAYRS_INVALID_ARG;
    if (lab->static_pct > 100u || lab->refill_min > 64u || lab->leaf_min > 64u || lab->leaf_wait > 64u || lab->flat_blocks_per_cu > 64u || lab->eager_light > 1u || lab->force_rccl > 1u || lab->gate_tree > 1u)
        return RAYRS_INVALID_ARG;
    if (lab->local_reserve != 0u && (lab->local_reserve < 8u || lab->local_reserve > 4096u)) return RAYRS_INVALID_ARG;
    if (lab->local_segment_items != 0u && lab->local_segment_items < 65536u) return RAYRS_INVALID_ARG;
    RAYRS_TRY(scene_quiesce(scene));
    scene->lab = *lab;
    if (scene->device >= 0) return scene_configure_traversal(scene);
    return RAYRS_OK;
}

int rayrs_lab_stack_need(rayrs_scene* scene, uint32_t which) {
    if (!scene || which > 2u || (which == 2u && !scene->flat.has_hot)) return RAYRS_INVALID_ARG;
    return (int)scene->stack_depth((int)which);
}

uint32_t rayrs_frame_sample_chunk(uint32_t x_pixels, uint32_t y_pixels, uint32_t spp, uint32_t requested) {
    if (spp == 0) return 0;
    uint64_t chunk = requested ? requested : 4u;
    const TileShare ts = tile_share(x_pixels, y_pixels, 0u, 1u);
    const uint64_t pixels = (uint64_t)ts.tiles_x * ts.tiles_y * 64u;  // whole 8x8 tiles
    while (chunk < spp && pixels * ((spp + chunk - 1) / chunk) > (1ull << 30)) chunk *= 2;
    return chunk >= spp ? 0u : (uint32_t)chunk;  // 0 = one sequential sum per pixel (the reference's order)
}

uint32_t rayrs_abi_version(void) { return RAYRS_ABI_VERSION; }

uint32_t rayrs_abi_layout(uint32_t* out, uint32_t cap) {
    std::vector<uint32_t> t;
    t.push_back(RAYRS_ABI_VERSION);  // (a binding that validates itself against this table fails on a version change too)
#define RAYRS_STRUCT(T, N) t.push_back((uint32_t)sizeof(T)), t.push_back(N)
#define RAYRS_FIELD(T, F) t.push_back((uint32_t)offsetof(T, F))
    RAYRS_STRUCT(rayrs_material, 7);
    RAYRS_FIELD(rayrs_material, kind), RAYRS_FIELD(rayrs_material, metallic), RAYRS_FIELD(rayrs_material, color);
    RAYRS_FIELD(rayrs_material, spec_color), RAYRS_FIELD(rayrs_material, alpha), RAYRS_FIELD(rayrs_material, ior);
    RAYRS_FIELD(rayrs_material, r0);
    RAYRS_STRUCT(rayrs_emission, 4);
    RAYRS_FIELD(rayrs_emission, emissive), RAYRS_FIELD(rayrs_emission, pad), RAYRS_FIELD(rayrs_emission, strength);
    RAYRS_FIELD(rayrs_emission, color);
    RAYRS_STRUCT(rayrs_camera, 9);
    RAYRS_FIELD(rayrs_camera, origin), RAYRS_FIELD(rayrs_camera, e_x), RAYRS_FIELD(rayrs_camera, e_y);
    RAYRS_FIELD(rayrs_camera, z), RAYRS_FIELD(rayrs_camera, width), RAYRS_FIELD(rayrs_camera, height);
    RAYRS_FIELD(rayrs_camera, ppc), RAYRS_FIELD(rayrs_camera, x_pixels), RAYRS_FIELD(rayrs_camera, y_pixels);
    RAYRS_STRUCT(rayrs_scene_info_t, 26);
    RAYRS_FIELD(rayrs_scene_info_t, n_objects), RAYRS_FIELD(rayrs_scene_info_t, n_interior);
    RAYRS_FIELD(rayrs_scene_info_t, n_prims), RAYRS_FIELD(rayrs_scene_info_t, root_ref);
    RAYRS_FIELD(rayrs_scene_info_t, depth), RAYRS_FIELD(rayrs_scene_info_t, compact);
    RAYRS_FIELD(rayrs_scene_info_t, n_surfaces), RAYRS_FIELD(rayrs_scene_info_t, node_bytes);
    RAYRS_FIELD(rayrs_scene_info_t, prim_bytes), RAYRS_FIELD(rayrs_scene_info_t, device_bytes);
    RAYRS_FIELD(rayrs_scene_info_t, root_box), RAYRS_FIELD(rayrs_scene_info_t, build_seconds);
    RAYRS_FIELD(rayrs_scene_info_t, n_wide), RAYRS_FIELD(rayrs_scene_info_t, wide_root_ref);
    RAYRS_FIELD(rayrs_scene_info_t, wide_depth), RAYRS_FIELD(rayrs_scene_info_t, local_pool);
    RAYRS_FIELD(rayrs_scene_info_t, gate_n_wide), RAYRS_FIELD(rayrs_scene_info_t, gate_root_ref);
    RAYRS_FIELD(rayrs_scene_info_t, gate_depth);
    RAYRS_FIELD(rayrs_scene_info_t, hot_n_wide), RAYRS_FIELD(rayrs_scene_info_t, hot_root_ref);
    RAYRS_FIELD(rayrs_scene_info_t, hot_depth), RAYRS_FIELD(rayrs_scene_info_t, hot_first);
    RAYRS_FIELD(rayrs_scene_info_t, hot_count), RAYRS_FIELD(rayrs_scene_info_t, hot_pad);
    RAYRS_FIELD(rayrs_scene_info_t, hot_box);
    RAYRS_STRUCT(rayrs_render_params, 9);
    RAYRS_FIELD(rayrs_render_params, spp), RAYRS_FIELD(rayrs_render_params, max_bounces);
    RAYRS_FIELD(rayrs_render_params, seed), RAYRS_FIELD(rayrs_render_params, sample_chunk);
    RAYRS_FIELD(rayrs_render_params, tile_rank), RAYRS_FIELD(rayrs_render_params, tile_ranks);
    RAYRS_FIELD(rayrs_render_params, out_format), RAYRS_FIELD(rayrs_render_params, count_work);
    RAYRS_FIELD(rayrs_render_params, fast_traversal);
    RAYRS_STRUCT(rayrs_render_stats, 33);
    RAYRS_FIELD(rayrs_render_stats, rays), RAYRS_FIELD(rayrs_render_stats, paths);
    RAYRS_FIELD(rayrs_render_stats, nan_pixels), RAYRS_FIELD(rayrs_render_stats, neg_pixels);
    RAYRS_FIELD(rayrs_render_stats, interior_visits), RAYRS_FIELD(rayrs_render_stats, tri_tests);
    RAYRS_FIELD(rayrs_render_stats, sphere_tests), RAYRS_FIELD(rayrs_render_stats, plane_tests);
    RAYRS_FIELD(rayrs_render_stats, escaped_paths), RAYRS_FIELD(rayrs_render_stats, step_wave);
    RAYRS_FIELD(rayrs_render_stats, step_lane), RAYRS_FIELD(rayrs_render_stats, inner_wave);
    RAYRS_FIELD(rayrs_render_stats, leaf_wave), RAYRS_FIELD(rayrs_render_stats, interior_ticks);
    RAYRS_FIELD(rayrs_render_stats, leaf_ticks), RAYRS_FIELD(rayrs_render_stats, kernel_ms);
    RAYRS_FIELD(rayrs_render_stats, total_ms), RAYRS_FIELD(rayrs_render_stats, kernel_launches);
    RAYRS_FIELD(rayrs_render_stats, trace_ms), RAYRS_FIELD(rayrs_render_stats, refill_ticks);
    RAYRS_FIELD(rayrs_render_stats, surface_hits), RAYRS_FIELD(rayrs_render_stats, direct_rays);
    RAYRS_FIELD(rayrs_render_stats, hit_ms), RAYRS_FIELD(rayrs_render_stats, miss_ms);
    RAYRS_FIELD(rayrs_render_stats, local_pool), RAYRS_FIELD(rayrs_render_stats, exact_walk);
    RAYRS_FIELD(rayrs_render_stats, hot_group), RAYRS_FIELD(rayrs_render_stats, stats_pad);
    RAYRS_FIELD(rayrs_render_stats, pre_rays), RAYRS_FIELD(rayrs_render_stats, pre_root_records);
    RAYRS_FIELD(rayrs_render_stats, hot_lane);
    RAYRS_FIELD(rayrs_render_stats, hot_prim_tests), RAYRS_FIELD(rayrs_render_stats, hot_tri_divided);
    RAYRS_STRUCT(rayrs_tuning, 2);
    RAYRS_FIELD(rayrs_tuning, pool_slots), RAYRS_FIELD(rayrs_tuning, local_pool);
    RAYRS_STRUCT(rayrs_film_params, 7);
    RAYRS_FIELD(rayrs_film_params, sample_chunk), RAYRS_FIELD(rayrs_film_params, max_bounces);
    RAYRS_FIELD(rayrs_film_params, seed), RAYRS_FIELD(rayrs_film_params, tile_rank);
    RAYRS_FIELD(rayrs_film_params, tile_ranks), RAYRS_FIELD(rayrs_film_params, fast_traversal);
    RAYRS_FIELD(rayrs_film_params, pad);
    RAYRS_STRUCT(rayrs_film_status, 10);
    RAYRS_FIELD(rayrs_film_status, samples), RAYRS_FIELD(rayrs_film_status, full_chunks);
    RAYRS_FIELD(rayrs_film_status, rays), RAYRS_FIELD(rayrs_film_status, paths);
    RAYRS_FIELD(rayrs_film_status, nan_pixels), RAYRS_FIELD(rayrs_film_status, neg_pixels);
    RAYRS_FIELD(rayrs_film_status, unconverged), RAYRS_FIELD(rayrs_film_status, nonfinite);
    RAYRS_FIELD(rayrs_film_status, closed), RAYRS_FIELD(rayrs_film_status, pad);
#undef RAYRS_STRUCT
#undef RAYRS_FIELD
    for (uint32_t i = 0; i < cap && i < t.size(); i++) out[i] = t[i];
    return (uint32_t)t.size();
}

// ------------------------------------------------------------------ Camera

int rayrs_camera_new(const double origin[3], const double up[3], const double lookat[3], double fov, double width,
                     double height, uint32_t ppi, rayrs_camera* out) {
    return camera_new(origin, up, lookat, fov, width, height, ppi, out);
}

// ------------------------------------------------------------------ render

int rayrs_render_launch(rayrs_scene* scene, const rayrs_camera* camera, const rayrs_render_params* params,
                        void* out_device, void* hip_stream) {
    if (!out_device) return RAYRS_INVALID_ARG;
    return render_enqueue(scene, camera, params, 0u, nullptr, out_device, hip_stream);
}

int rayrs_render_finish(rayrs_scene* scene, rayrs_render_stats* stats) {
    if (!scene) return RAYRS_INVALID_ARG;
    return render_finish(scene, stats);
}

int rayrs_render(rayrs_scene* scene, const rayrs_camera* camera, const rayrs_render_params* params, void* out_host,
                 rayrs_render_stats* stats) {
    if (!scene || !camera || !params || !out_host) return RAYRS_INVALID_ARG;
    if (scene->device < 0) return RAYRS_NO_DEVICE;
    HIP_TRY(hipSetDevice(scene->device));
    const size_t bytes = frame_bytes(camera->x_pixels, camera->y_pixels, params->out_format);
    DevBuf d_out;
    HIP_TRY(d_out.upload(out_host, bytes));  // pixels of other ranks' tiles keep the caller's values
    RAYRS_TRY(rayrs_render_launch(scene, camera, params, d_out.as<>(), nullptr));
    RAYRS_TRY(rayrs_render_finish(scene, stats));
    HIP_TRY(d_out.download(out_host, bytes));
    return RAYRS_OK;
}

}  // extern "C"
