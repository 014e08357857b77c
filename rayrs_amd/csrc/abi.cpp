// abi.cpp -- the extern "C" boundary declared in include/rayrs_hip.h: the entry points, a scene's lifetime, and a render as
// plan_frame (arithmetic only), reserve, enqueue.  The device self tests of rayrs_selftest.h are in selftest.cpp.
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
#include "film.h"
#include "kernels.h"
#include "local_pool.h"
#include "rayrs_lab.h"
#include "scene_host.hpp"
#include "scene_internal.hpp"
#include "wavefront.h"

using namespace rayrs;

namespace {
thread_local std::string g_last_error;
constexpr uint32_t TRAV_STACK_LDS = 12;
constexpr uint32_t TRAV_HOT_BYTES = 14u * 1024u;
// The trees the default walk reads: a lane's leaf groups wait in a queue of LEAFQ entries behind its stack
// (device_path.h trav_interior_step_defer), so its stack holds interior records only -- 8 entries in LDS serve what 12
// served with the leaves among them -- and the records kept in LDS give up the other 4 KiB of the queue's 8.
constexpr uint32_t FLAT_BLOCKS_PER_CU_MIN = 8, FLAT_BLOCKS_PER_CU_MAX = 24;  // the gen / hit / miss kernels' common grid (rayrs_lab_tuning.flat_blocks_per_cu)
constexpr uint32_t TRAV_STACK_LDS_DEFER = 8;
constexpr uint32_t TRAV_HOT_BYTES_DEFER = 10u * 1024u;
}  // namespace

namespace rayrs {
void set_last_error(const std::string& text) { g_last_error = text; }
int hip_fail(hipError_t e, const char* what) {
    g_last_error = std::string(what) + ": " + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? RAYRS_OOM : RAYRS_HIP_ERROR;
}
int scene_settle(rayrs_scene* scene) {
    HIP_TRY(hipSetDevice(scene->device));
    if (scene->pending && scene->last_stream) {
        HIP_TRY(hipStreamSynchronize(scene->last_stream));
        scene->pending = false;
    }
    return RAYRS_OK;
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

// Sizes the traversal workgroup's LDS from the tree and the scene's tuning, and asks the runtime how
// many such workgroups fit a CU.  A workgroup's LDS: the first stack_lds entries of each lane's stack
// (deeper entries overflow to HBM; on the 1M-triangle scene 99.4 % of visits happen with at most 7
// pending), 4 KiB of window lists, and the hot_records largest wide records.  13 + 4 + 14 KiB (the default walk's trees: 17 KiB with the lanes' leaf queues + 4 + 10) lets
// five workgroups (the kernel's launch bound) share a CU's 160 KiB.
// The kernel's dynamic-LDS limit belongs to the kernel on a device, not to a scene, and the scenes of a process share
// it: it is only ever raised (wf_trav_raise_lds), so it ends at no less than the largest size among the trees this scene has.
static int scene_configure_traversal(rayrs_scene* s) {
    const FlatScene& f = s->flat;
    for (int x = 0; x < 3; x++) {
        if (x == 2 && !f.has_hot) continue;
        const WalkTree& t = s->tree(x);
        rayrs_scene::Walk& w = s->trav[x];
        const uint32_t depth = t.depth ? t.depth : 1;
        w.leafq = x == 0 ? 0u : TRAV_LEAFQ;  // ([0] is the fast walk's tree; [1] is walked either way, [2] by the default walk only)
        uint32_t want = s->lab.stack_lds ? s->lab.stack_lds : (w.leafq ? TRAV_STACK_LDS_DEFER : TRAV_STACK_LDS);
        w.stack_lds = want < depth ? want : depth;
        const uint32_t rec_bytes = f.compact ? (uint32_t)sizeof(Node4F32) + 16u : (uint32_t)sizeof(Node4F64) + 16u;
        uint32_t hot = (w.leafq ? TRAV_HOT_BYTES_DEFER : TRAV_HOT_BYTES) / rec_bytes;
        if (s->lab.hot_records == 0xffffffffu) hot = 0;
        else if (s->lab.hot_records) hot = s->lab.hot_records < WIDE_FRONT ? s->lab.hot_records : WIDE_FRONT;
        w.hot_records = hot < t.n() ? hot : t.n();
        const uint32_t lds = wf_trav_lds_bytes(f.compact, w.stack_lds, w.leafq, w.hot_records);
        HIP_TRY(wf_trav_raise_lds(f.compact, lds));  // (before the query, which is about a launch with this much)
        HIP_TRY(wf_trav_occupancy(f.compact, lds, &w.blocks_per_cu));
        if (w.blocks_per_cu < 1) w.blocks_per_cu = 1;
    }
    return RAYRS_OK;
}

// The gating boxes of a walk tree of at most one record, as kernel arguments of local_pool.hip (LocalScene).
constexpr uint32_t LOCAL_SEGMENT_ITEMS = 1u << 27;  // items per launch of the local-pool kernel
constexpr uint32_t LOCAL_MAX_SEGMENTS = 64;
static void scene_configure_local(rayrs_scene* s) {
    const FlatScene& f = s->flat;
    LocalScene& ls = s->local;
    std::memset(&ls, 0, sizeof(ls));
    s->local_ok = false;
    const WalkTree& t = f.gate;  // (the groups behind their gating boxes: this route makes neither of the default walk's bets)
    if (t.n() > 1 || f.n_prims() == 0 || f.n_prims() > LP_MAX_PRIMS || s->surfaces.size() > LP_MAX_PRIMS) return;
    auto add_gate = [&](const double* box, uint32_t ref) {
        if (ref_kind(ref) != REF_RANGE) return false;
        const uint32_t g = ls.n_gates++;
        for (int i = 0; i < 6; i++) ls.box[g][i] = box[i];
        ls.first[g] = ref_first(ref);
        ls.count[g] = ref_count(ref);
        return true;
    };
    if (t.n() == 0) {  // the root group behind the root Node's box (trav_init)
        if (!add_gate(f.root_box, t.root_ref)) return;
    } else {
        if (ref_kind(t.root_ref) != REF_INTERIOR) return;
        for (uint32_t k = 0; k < 4; k++) {
            const uint32_t ref = t.ref[k];
            if (ref_kind(ref) == REF_NONE) continue;
            if (!add_gate(&t.box[(size_t)k * 6], ref)) return;  // an interior slot: not a one-record tree
        }
    }
    uint32_t covered = 0;
    for (uint32_t g = 0; g < ls.n_gates; g++) covered += ls.count[g];
    if (covered != f.n_prims()) return;
    ls.n_records = t.n();
    ls.n_prims = f.n_prims();
    for (const SurfaceDev& sf : s->surfaces) ls.kind_mask |= 1u << (uint32_t)sf.kind;
    s->local_ok = true;
}

extern "C++" int rayrs::scene_upload(rayrs_scene* s) {
    HIP_TRY(hipSetDevice(s->device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, s->device));
    s->cu_count = prop.multiProcessorCount;
    const FlatScene& f = s->flat;
    for (int x = 0; x < 3; x++) {
        const WalkTree& t = s->tree(x);
        if (x == 2 && !f.has_hot) continue;
        HIP_TRY(s->trav[x].d_nodes.upload(t.node_bytes.data(), t.node_bytes.size()));
    }
    if (f.has_hot) HIP_TRY(s->d_hot.upload(&f.hot, sizeof(HotGroupDev)));
    HIP_TRY(s->d_prims.upload(f.prim_bytes.data(), f.prim_bytes.size()));
    HIP_TRY(s->d_surfaces.upload(s->surfaces.data(), s->surfaces.size() * sizeof(SurfaceDev)));
    HIP_TRY(s->d_hdri.upload(f.hdri_quads.data(), f.hdri_quads.size() * sizeof(float)));
    HIP_TRY(s->d_counters.reserve(sizeof(Counters)));
    for (auto& e : s->ev) HIP_TRY(e.create());
    s->device_bytes = f.walk.node_bytes.size() + f.gate.node_bytes.size() + (f.has_hot ? f.gate_hot.node_bytes.size() : 0) + f.prim_bytes.size() + s->surfaces.size() * sizeof(SurfaceDev) +
                      f.hdri_quads.size() * sizeof(float);
    RAYRS_TRY(scene_configure_traversal(s));
    HIP_TRY(s->pool.d_ctl.reserve(sizeof(WfCtl)));
    HIP_TRY(s->pool.h_live.alloc(2 * sizeof(uint32_t)));
    for (auto& e : s->pool.ev_batch) HIP_TRY(e.create());
    HIP_TRY(s->d_next_item.reserve(sizeof(unsigned long long)));
    if (s->local_ok) {
        HIP_TRY(lp_configure());
        // (from about 13 primitives and surface rows up three workgroups' LDS no longer fit a CU: ask, do not assume)
        HIP_TRY(lp_occupancy(s->flat.compact, s->local.n_prims, (uint32_t)s->surfaces.size(), &s->local_blocks_per_cu));
        if (s->local_blocks_per_cu < 1) s->local_blocks_per_cu = 1;
        if (s->local_blocks_per_cu > (int)LP_WPS) s->local_blocks_per_cu = (int)LP_WPS;
        HIP_TRY(s->d_local_items.reserve(LOCAL_MAX_SEGMENTS * sizeof(unsigned long long)));
    }
    return RAYRS_OK;
}

int rayrs_scene_new(const rayrs_objects* objs, double z_near, double z_far, int heuristic, uint32_t splits,
                    uint32_t hdri_w, uint32_t hdri_h, const float* hdri_rgb, int device, rayrs_scene** out) {
    RAYRS_GUARDED({
    if (!objs || !out) return RAYRS_INVALID_ARG;
    *out = nullptr;
    std::unique_ptr<rayrs_scene> s(new rayrs_scene());
    RAYRS_TRY(build_flat_scene(objs->list, z_near, z_far, heuristic, splits, hdri_w, hdri_h, hdri_rgb, &s->flat));
    // Every traversal lane gets a stack of WalkTree::depth entries (12 in LDS, the rest in HBM: 1.3 MB per entry on a
    // 256-CU device).  The reference recurses as deep as its tree; a tree that needs more than 4096 pending
    // entries (a chain of thousands of nested objects) is refused instead of allocating gigabytes for it.
    if (std::max(s->flat.walk.depth, s->flat.gate.depth) > 4096u) {
        g_last_error = "walk tree needs " + std::to_string(std::max(s->flat.walk.depth, s->flat.gate.depth)) + " stack entries (limit 4096)";
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

// A render in flight ends before any member releases what it uses (nothing here touches rayrs_last_error).
rayrs_scene::~rayrs_scene() {
    if (device < 0) return;
    (void)hipSetDevice(device);
    if (pending && last_stream) (void)hipStreamSynchronize(last_stream);
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
    HIP_TRY(scene->d_counters.download(&c, sizeof(c)));
    for (int i = 0; i < 16; i++) out[i] = c.lab_ticks[i];
    return RAYRS_OK;
}
#endif

// A timed round r owns four events, pool.ev_round[4 r + k]: k = 0 before its traversal kernel, 1 behind it, 2 behind the hit
// kernel, 3 behind the miss kernel (the local-pool route: 0 and 1 around a segment's one launch).  round_event records one
// of them (and creates the round's four the first time); round_ms reads the three intervals back after the frame.
static int round_event(rayrs_scene::Pool& pl, uint32_t r, uint32_t k, hipStream_t stream) {
    while (pl.ev_round.size() < 4 * (size_t)(r + 1)) {
        Event e;
        HIP_TRY(e.create());
        pl.ev_round.push_back(std::move(e));
    }
    HIP_TRY(hipEventRecord(pl.ev_round[4 * (size_t)r + k], stream));
    return RAYRS_OK;
}

static int round_ms(const rayrs_scene* scene, uint32_t r, float ms[3]) {
    const Event* e = &scene->pool.ev_round[4 * (size_t)r];
    ms[1] = ms[2] = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms[0], e[0], e[1]));
    if (scene->last_local) return RAYRS_OK;  // one kernel per segment
    HIP_TRY(hipEventElapsedTime(&ms[1], e[1], e[2]));
    HIP_TRY(hipEventElapsedTime(&ms[2], e[2], e[3]));
    return RAYRS_OK;
}

// rayrs_lab.h: HIP-event times of the last render's path rounds, three per round (traversal, hit, miss kernel; the
// local-pool route: its launch, 0, 0).  Returns the number of rounds; writes at most cap_rounds of them.
extern "C" int rayrs_lab_round_ms(rayrs_scene* scene, float* out, uint32_t cap_rounds) {
    if (!scene || scene->device < 0 || scene->pending) return RAYRS_INVALID_ARG;
    HIP_TRY(hipSetDevice(scene->device));
    for (uint32_t r = 0; r < scene->pool.timed_rounds && r < cap_rounds && out; r++) RAYRS_TRY(round_ms(scene, r, out + 3 * r));
    return (int)scene->pool.timed_rounds;
}

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

extern "C++" SceneDev rayrs::make_scene_dev(const rayrs_scene* s, bool exact) {
    SceneDev sc;
    std::memset(&sc, 0, sizeof(sc));
    const int which = s->walk_index(exact);
    const WalkTree& t = s->tree(which);
    const rayrs_scene::Walk& w = s->trav[which];
    sc.hot = which == 2 ? s->d_hot.as<HotGroupDev>() : nullptr;
    sc.nodes = w.d_nodes.as<>();
    sc.prims = s->d_prims.as<>();
    sc.surfaces = s->d_surfaces.as<SurfaceDev>();
    sc.hdri = s->d_hdri.as<float>();
    sc.hdri_w = s->flat.hdri_w;
    sc.hdri_h = s->flat.hdri_h;
    sc.hdri_wm1 = (double)(s->flat.hdri_w - 1u);
    sc.hdri_hm1 = (double)(s->flat.hdri_h - 1u);
    sc.root_ref = t.root_ref;
    sc.stack_depth = t.depth ? t.depth : 1;
    sc.stack_lds = w.stack_lds;
    sc.hot_records = w.hot_records;
    sc.leafq = w.leafq;
    sc.n_surfaces = (uint32_t)s->surfaces.size();
    for (int i = 0; i < 6; i++) sc.root_box[i] = s->flat.root_box[i];
    sc.t0 = s->flat.t0;
    sc.t1 = s->flat.t1;
    sc.exact = exact ? 1u : 0u;
    return sc;
}

// The fast walk's leaf boxes are a bet on the reference's arithmetic that was measured to hold for rays from nearby and
// to fail, a few times in 10^4, for rays aimed along a primitive's plane from far away (include/rayrs_hip.h
// fast_traversal; profiles/r04_tight_leaves.txt).  What decides is the distance in PRIMITIVE sizes (the error of the
// computed hit point is about eps * distance / angle against a widening of 1/64 of the primitive): failures were seen from
// 6,000 primitive sizes up, none within 4,000 (sheets of 6 ... 400 quads per side: scripts/fuzz_traversal.py).
// A frame whose camera is farther from the root Node's box than RAYRS_FAR_DIAGONALS times that box's diagonal, or than
// RAYRS_FAR_PRIMITIVES times the scene's small primitives (the 5th percentile of their largest extents), takes the
// default walk whatever was asked (rayrs_render_stats.exact_walk says which walk a frame took).  This guards PRIMARY
// rays only: a bounced ray from a large surface to a finely tessellated one (the headline scene's floor to its mesh)
// is thousands of small-primitive sizes long and makes the bet all the same -- the fast walk stays a bet.
constexpr double RAYRS_FAR_DIAGONALS = 8.0;
constexpr double RAYRS_FAR_PRIMITIVES = 4096.0;
static bool camera_is_far(const rayrs_scene* s, const rayrs_camera* c) {
    const double* b = s->flat.root_box;
    double d2 = 0.0, e2 = 0.0;
    for (int a = 0; a < 3; a++) {
        const double lo = b[2 * a], hi = b[2 * a + 1], o = c->origin[a];
        const double out = o < lo ? lo - o : (o > hi ? o - hi : 0.0);
        d2 += out * out;
        e2 += (hi - lo) * (hi - lo);
    }
    // (a box or an origin that is not a number compares false: the walk that was asked for, as for any other frame)
    const double small = s->flat.small_extent;
    return d2 > RAYRS_FAR_DIAGONALS * RAYRS_FAR_DIAGONALS * e2 || (small > 0.0 && d2 > RAYRS_FAR_PRIMITIVES * RAYRS_FAR_PRIMITIVES * small * small);
}

extern "C++" FrameWalk rayrs::frame_walk(const rayrs_scene* s, const rayrs_camera* c, uint32_t fast_traversal) {
    return FrameWalk{s->local_ok && s->tuning.local_pool != 1u, fast_traversal == 0u || camera_is_far(s, c)};
}

extern "C++" CameraDev rayrs::make_camera_dev(const rayrs_camera* c) {
    CameraDev cam;
    std::memset(&cam, 0, sizeof(cam));
    for (int i = 0; i < 3; i++) {
        cam.origin[i] = c->origin[i];
        cam.e_x[i] = c->e_x[i];
        cam.e_y[i] = c->e_y[i];
        cam.z[i] = c->z[i];
    }
    cam.width = c->width;
    cam.height = c->height;
    cam.ppc = (double)c->ppc;  // `self.ppc as f64`, lib.rs:206
    cam.W = c->x_pixels;
    cam.H = c->y_pixels;
    return cam;
}

// The traversal kernel's launch settings on a pool of np slots, for a render and for rayrs_test_trace alike: its scheduling
// thresholds (rayrs_lab.h) and the windows dealt round robin into rp, its grid as the result.
extern "C++" uint32_t rayrs::trav_settings(const rayrs_scene* s, bool exact, uint32_t np, RenderDev& rp) {
    const rayrs_lab_tuning& lab = s->lab;
    rp.refill_min = lab.refill_min ? lab.refill_min : 52u;
    // (a leaf phase once this many lanes stand on a leaf: 24 where a leaf is one primitive -- the fast walk's tree: 612 -> 604 ms
    // of traversal on the headline frame against 32 --, 32 where it is a group of up to four -- the default walk: 988 -> 962 ms
    // against 24)
    rp.leaf_min = lab.leaf_min ? lab.leaf_min : (exact ? 48u : lab.gate_tree ? 32u : 24u);
    // (the default walk: its lanes walk on while their leaf groups wait, so a leaf phase may wait for more of them -- or for
    // leaf_wait lanes that can do nothing else; scripts/sim/walk_sched_sim.py, swept on the GPU: profiles/r06_leaf_queue.txt)
    rp.leaf_wait = lab.leaf_wait ? lab.leaf_wait : 16u;
    // (pre-tested rays -- a scene with a hot group, wavefront.hip finish_rays -- wanted a refill_min of 56 while a lane stood idle
    // on its leaf: 664 -> 659 ms of traversal, profiles/r06_tuning_sweep.txt; with the leaf groups set aside 52 is best again:
    // 626 -> 619 ms, profiles/r06_leaf_queue.txt)
    uint32_t trav_bpc = (uint32_t)s->trav[s->walk_index(exact)].blocks_per_cu;
    if (lab.trav_blocks_per_cu && lab.trav_blocks_per_cu < trav_bpc) trav_bpc = lab.trav_blocks_per_cu;
    const uint32_t blocks = (uint32_t)s->cu_count * trav_bpc;
    // whole round-robin rounds covering about static_pct % of the pool's windows
    const uint32_t static_pct = lab.static_pct ? lab.static_pct : 50u;  // (rayrs_lab_set: at most 100)
    const uint64_t n_waves = (uint64_t)blocks * 4u;
    rp.static_windows = (uint32_t)((uint64_t)(np / wf_window_slots()) * static_pct / 100u / n_waves * n_waves);
    return blocks;
}

// A pool of np slots (whole windows) in one block -- the slot records, the light entries, the state bytes -- walked by
// trav_blocks workgroups whose stacks overflow into `spill`.
extern "C++" WfDev rayrs::pool_wf(const DevBuf& block, uint32_t np, const DevBuf& ctl, uint32_t trav_blocks, const DevBuf& spill) {
    WfDev wf;
    std::memset(&wf, 0, sizeof(wf));
    wf.slots = block.as<PathSlot>();
    wf.light = reinterpret_cast<double*>(wf.slots + np);
    wf.state = reinterpret_cast<uint8_t*>(wf.light + (size_t)np * 4u);
    wf.ctl = ctl.as<WfCtl>();
    wf.np = np;
    wf.trav_threads = trav_blocks * 256u;
    wf.stack_spill = spill.as<uint32_t>();
    return wf;
}

// What a frame is, worked out before anything is allocated or enqueued: plan_frame calls nothing in HIP.
struct FramePlan {
    SceneDev sc;
    CameraDev cam;
    RenderDev rp;  // complete but for `partial`
    bool exact, eager_light, use_local;  // use_local: the local-pool route (else the streaming route)
    uint64_t partial_need;     // item sums the frame needs at a time
    // the local-pool route: launches over segments of seg_tiles whole tiles, by local_blocks workgroups
    uint64_t tile_items, seg_tiles, seg_items;
    uint32_t local_blocks;  // (0: not this route)
    // the streaming route: live_total slots in a pool of np, the traversal grid, the gen / hit / miss kernels' common grid
    uint64_t live_total;
    uint32_t np, trav_blocks, flat_blocks;  // (np 0, and with it flat_blocks and spill_words: not this route)
    size_t spill_words;
    // a film pass (rayrs_film_render): film_accumulate_kernel takes the resolve kernel's place
    bool is_film;
    FilmPassDev film;
};

// The frame's items: the (pixel, chunk) pairs of this rank's 8x8 tiles (the caller refuses 2^32 of them and more) -- or,
// for a film pass over a tile list, of the list's tiles.
static RenderDev make_render_dev(const rayrs_scene* scene, const rayrs_camera* camera, const rayrs_render_params* params, uint32_t sample0,
                                 const FilmPassDev* film, void* out_device) {
    RenderDev rp;
    std::memset(&rp, 0, sizeof(rp));
    rp.spp = params->spp;
    rp.sample0 = sample0;
    rp.max_bounces = params->max_bounces;
    rp.seed = params->seed;
    rp.chunk = (params->sample_chunk == 0 || params->sample_chunk >= params->spp) ? params->spp : params->sample_chunk;
    rp.nchunks = (rp.spp + rp.chunk - 1) / rp.chunk;
    const TileShare ts = tile_share(camera->x_pixels, camera->y_pixels, params->tile_rank, params->tile_ranks);
    rp.tile_rank = ts.tile_rank, rp.tile_ranks = ts.tile_ranks;
    rp.tiles_x = ts.tiles_x, rp.tiles_y = ts.tiles_y;
    rp.n_local_tiles = ts.n_local_tiles;
    if (film && film->list) {  // (at most the share's tiles)
        if (film->n_list < rp.n_local_tiles) rp.n_local_tiles = film->n_list;
        rp.tile_list = film->list;
    }
    rp.total_items = (uint64_t)rp.n_local_tiles * rp.nchunks * 64ull;
    rp.inv_nchunks = 1.0 / (double)rp.nchunks;
    rp.inv_tiles_x = 1.0 / (double)rp.tiles_x;
    rp.count_work = params->count_work ? 1u : 0u;
    rp.out_format = params->out_format;
    rp.out = out_device;
    rp.counters = scene->d_counters.as<Counters>();
    rp.next_item = scene->d_next_item.as<unsigned long long>();
    return rp;
}

static int plan_frame(const rayrs_scene* scene, const rayrs_camera* camera, const rayrs_render_params* params, uint32_t sample0,
                      const FilmPassDev* film, void* out_device, FramePlan& p) {
    const rayrs_lab_tuning& lab = scene->lab;
    RenderDev& rp = p.rp = make_render_dev(scene, camera, params, sample0, film, out_device);
    if (rp.total_items >= (1ull << 32)) return RAYRS_UNSUPPORTED;
    // Item sums: 24 bytes per (pixel, chunk) item, added per pixel in chunk order by the resolve kernel.  The streaming
    // kernels finish items in no particular order, so the array covers the frame.  The local-pool route renders the frame
    // as a sequence of launches over segments of whole tiles and resolves each segment behind its launch: one segment's
    // worth is all it needs (config 4: 3.2 GB instead of 25.8).
    const FrameWalk walk = frame_walk(scene, camera, params->fast_traversal);
    p.use_local = walk.use_local, p.exact = walk.exact;
    p.tile_items = (uint64_t)rp.nchunks * 64u;
    uint64_t seg_want = lab.local_segment_items ? lab.local_segment_items : LOCAL_SEGMENT_ITEMS;
    // (a frame stays within LOCAL_MAX_SEGMENTS launches: larger segments rather than a refused frame)
    if ((rp.total_items + seg_want - 1) / seg_want > LOCAL_MAX_SEGMENTS) seg_want = (rp.total_items + LOCAL_MAX_SEGMENTS - 1) / LOCAL_MAX_SEGMENTS;
    p.seg_tiles = (seg_want + p.tile_items - 1) / p.tile_items > 0 ? (seg_want + p.tile_items - 1) / p.tile_items : 1;
    p.seg_items = p.seg_tiles * p.tile_items;
    p.partial_need = p.use_local && p.seg_items < rp.total_items ? p.seg_items : rp.total_items;
    if (p.use_local && p.seg_items >= (1ull << 32)) return RAYRS_UNSUPPORTED;  // (one tile's chunks alone: spp beyond 2^27)
    // LP_WPS workgroups of four waves per CU; fewer when the frame has fewer items than resident paths
    p.local_blocks = (uint32_t)scene->cu_count * (uint32_t)scene->local_blocks_per_cu;
    const uint64_t most_items = rp.total_items < p.seg_items ? rp.total_items : p.seg_items;
    const uint64_t want_blocks = (most_items + 4u * LP_PATHS_PER_WAVE - 1) / (4u * LP_PATHS_PER_WAVE);
    if (want_blocks < p.local_blocks) p.local_blocks = (uint32_t)(want_blocks ? want_blocks : 1);
    if (!p.use_local || rp.total_items == 0) p.local_blocks = 0;

    p.sc = make_scene_dev(scene, p.exact);
    p.cam = make_camera_dev(camera);

    // ---- path pool.  A traversal launch works through the whole pool, and its ramp-up
    // and drain are a fixed cost, so large pools win even when that leaves only one or two
    // items per slot -- up to the point where the hit and miss kernels lose more to the larger
    // footprint.  Swept on the headline frame with one-line slots: 24 M slots 1520 ms, 32 M 1516,
    // 48 M 1497, 64 M 1467, 96 M 1468, 128 M 1481, 192 M 1498 (round 1, 192-byte slots: 32 M).
    // Swept again on round 3's kernels (the traversal kernel faster, its fixed cost per launch the same): 64 M 1369 ms,
    // 80 M 1372, 96 M 1368, 112 M 1353, 128 M 1356, 160 M 1353, 192 M 1350: 112 M slots (18 GB of the 288 GB), 84 rounds.
    // And on round 6's (the hit kernel at three waves per SIMD, the cheap queries answered by the kernels that make the rays):
    // 80 M 1298 ms, 96 M 1290, 112 M 1276, 128 M 1278, 144 M 1267, 160 M 1250, 192 M 1250, 224 M 1246, 256 M 1242, 320 M 1242
    // (profiles/r06_leaf_queue.txt (12)): 256 M slots (43 GB), 52 rounds.
    // A frame should also last some tens of rounds, or filling and draining the pool is all it does: at most one
    // slot per 12 samples -- which is what a one-eighth tile share of the headline frame gets (44.7 M: 33.5 M 189 ms,
    // 48 M 184, 64 M 186).
    constexpr uint64_t POOL_MAX_SLOTS = 1ull << 28;
    uint64_t np64 = rp.total_items;
    if (np64 > POOL_MAX_SLOTS) np64 = POOL_MAX_SLOTS;
    {
        const uint64_t samples = rp.n_local_tiles * 64ull * rp.spp;
        const uint64_t by_work = samples / 12u > (1ull << 20) ? samples / 12u : (1ull << 20);
        if (np64 > by_work) np64 = by_work;
    }
    if (scene->tuning.pool_slots) np64 = scene->tuning.pool_slots;
    if (np64 > rp.total_items) np64 = rp.total_items;
    p.live_total = np64;
    const bool streaming = !p.use_local && rp.total_items > 0;  // (the local-pool route keeps its paths in LDS)
    p.np = streaming ? (uint32_t)((p.live_total + 1023ull) & ~1023ull) : 0u;  // whole windows
    p.trav_blocks = trav_settings(scene, p.exact, p.np, rp);
    p.spill_words = streaming ? stack_spill_words(p.sc, (uint64_t)p.trav_blocks * 256u) : 0;

    // A path's light lives in a side array and only while it is not +0 (wavefront.h PathSlot).  Where a surface
    // emits, paths do get light, and the hit and miss kernels request the side array's entry together with the
    // slot instead of after it.
    p.eager_light = lab.eager_light != 0u;
    for (const SurfaceDev& sf : scene->surfaces)
        if (sf.emit[0] != 0.0 || sf.emit[1] != 0.0 || sf.emit[2] != 0.0) p.eager_light = true;

    // the gen, hit and miss kernels run with this one grid, so wave w means the same windows in all three: one
    // wave per window, at most 8 ... 24 workgroups per CU (below)
    const uint32_t n_windows = p.np / wf_window_slots();
    p.flat_blocks = (n_windows + 3u) / 4u;
    // (8 ... 24 workgroups per CU, so that a wave has about nine windows: with the hit kernel at three resident workgroups
    // per CU a finer grid evens out the end of a launch -- hit 411 -> 404 ms on the headline's 218 k windows at 24 -- but
    // a wave that gets three windows spends its time on its first and last batch: config 3's 87 k windows want 8 or 9
    // (198 against 200.5 ms at 24); profiles/r06_leaf_queue.txt (9))
    uint32_t per_cu = lab.flat_blocks_per_cu;
    if (!per_cu) {
        per_cu = n_windows / (36u * (uint32_t)scene->cu_count);
        per_cu = per_cu < FLAT_BLOCKS_PER_CU_MIN ? FLAT_BLOCKS_PER_CU_MIN : per_cu > FLAT_BLOCKS_PER_CU_MAX ? FLAT_BLOCKS_PER_CU_MAX : per_cu;
    }
    const uint32_t flat_cap = (uint32_t)scene->cu_count * per_cu;
    if (p.flat_blocks > flat_cap) p.flat_blocks = flat_cap;
    return RAYRS_OK;
}

// ---- one launch per segment of the frame's items; a launch ends when its last path has (local_pool.hip)
static int enqueue_local(rayrs_scene* scene, const FramePlan& p, hipStream_t stream) {
    rayrs_scene::Pool& pl = scene->pool;
    const RenderDev& rp = p.rp;
    const uint64_t n_seg = (rp.total_items + p.seg_items - 1) / p.seg_items;
    for (uint64_t seg = 0; seg < n_seg; seg++) {
        LocalDev lp;
        lp.light = scene->d_local_light.as<double>();
        lp.next_item = scene->d_local_items.as<unsigned long long>() + seg;
        lp.item_base = seg * p.seg_items;
        lp.item_count = rp.total_items - lp.item_base < p.seg_items ? rp.total_items - lp.item_base : p.seg_items;
        RenderDev rseg = rp;
        rseg.partial_item0 = lp.item_base;
        const uint64_t share = lp.item_count / ((uint64_t)p.local_blocks * 4u * 16u);  // a sixteenth of a wave's share
        lp.reserve = (uint32_t)(share < 8u ? 8u : share > 256u ? 256u : share);
        if (scene->lab.local_reserve) lp.reserve = scene->lab.local_reserve;
        lp.pad = 0;
        RAYRS_TRY(round_event(pl, (uint32_t)seg, 0, stream));
        HIP_TRY(lp_launch(scene->flat.compact, rp.count_work != 0u, p.sc, scene->local, p.cam, rseg, lp, p.local_blocks, stream));
        RAYRS_TRY(round_event(pl, (uint32_t)seg, 1, stream));
        // the segment's tiles, resolved behind its launch (the next segment reuses the item-sum array)
        const uint32_t seg_lt0 = (uint32_t)(seg * p.seg_tiles), seg_n_lt = (uint32_t)(lp.item_count / p.tile_items);
        HIP_TRY(p.is_film ? launch_film_accumulate(p.cam, rseg, p.film, seg_lt0, seg_n_lt, stream) : launch_resolve(p.cam, rseg, seg_lt0, seg_n_lt, stream));
        pl.timed_rounds = (uint32_t)seg + 1;
    }
    scene->rounds = (uint32_t)n_seg;
    return RAYRS_OK;
}

static int enqueue_streaming(rayrs_scene* scene, const FramePlan& p, const WfDev& wf, hipStream_t stream) {
    rayrs_scene::Pool& pl = scene->pool;
    const RenderDev& rp = p.rp;
    uint32_t* h_live = pl.h_live.as<uint32_t>();
    HIP_TRY(wf_launch_init(wf, (uint32_t)p.live_total, stream));
    HIP_TRY(wf_launch_gen(scene->flat.compact, p.sc, p.cam, rp, wf, p.flat_blocks, stream));  // initial fill; later samples start in hit/miss
    h_live[0] = h_live[1] = (uint32_t)p.live_total;
    // Rounds are enqueued in batches; the live-slot count of batch b is read back while batch b+1 is
    // already queued, so the GPU never waits for the host.  Rounds behind the frame's last one find
    // live_slots == 0 and return at once; batches shrink from 16 rounds to 4 once fewer than an eighth of
    // the slots have work, so that at most 7 such rounds are queued after the end.
    constexpr uint32_t MAX_TIMED = 8192;
    uint32_t it = 0;
    uint32_t batch = 16;
    for (uint32_t b = 0;; b++) {
        for (uint32_t k = 0; k < batch; k++, it++) {
            const bool timed = it < MAX_TIMED;  // (rounds beyond the event pool: rayrs_render_finish extrapolates)
            if (timed) RAYRS_TRY(round_event(pl, it, 0, stream));
            HIP_TRY(wf_launch_trav(scene->flat.compact, rp.count_work != 0u, p.sc, rp, wf, p.trav_blocks, stream));
            if (timed) RAYRS_TRY(round_event(pl, it, 1, stream));
            HIP_TRY(wf_launch_hit(scene->flat.compact, p.eager_light, p.sc, p.cam, rp, wf, p.flat_blocks, stream));
            if (timed) RAYRS_TRY(round_event(pl, it, 2, stream));
            HIP_TRY(wf_launch_miss(scene->flat.compact, p.eager_light, p.sc, p.cam, rp, wf, p.flat_blocks, stream));
            if (timed) {
                RAYRS_TRY(round_event(pl, it, 3, stream));
                pl.timed_rounds = it + 1;
            }
        }
        HIP_TRY(hipMemcpyAsync(&h_live[b & 1u], &wf.ctl->live_slots, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipEventRecord(pl.ev_batch[b & 1u], stream));
        if (b > 0) {
            HIP_TRY(hipEventSynchronize(pl.ev_batch[(b - 1u) & 1u]));
            const uint64_t seen = h_live[(b - 1u) & 1u];
            if (seen == 0u) break;
            batch = seen * 8u < p.live_total ? 4u : 16u;
        }
        if (it > (1u << 26)) {
            g_last_error = "path rounds did not terminate";
            return RAYRS_HIP_ERROR;
        }
    }
    scene->rounds = it;
    return RAYRS_OK;
}

// A frame, or a film's pass: the samples sample0 .. sample0 + params->spp - 1 of every pixel of the share, summed per chunk
// of that window.  film == nullptr: the chunk sums are resolved into out_device (rayrs_render_launch, sample0 = 0); else
// they are added to the film's records and out_device is not used.  A film pass with a tile list covers the list's tiles
// only, each from its own sample count (sample0 is not used): the plan -- items, pool, grids -- is sized by the list.
extern "C++" int rayrs::render_enqueue(rayrs_scene* scene, const rayrs_camera* camera, const rayrs_render_params* params, uint32_t sample0,
                                       const FilmPassDev* film, void* out_device, void* hip_stream) {
    RAYRS_GUARDED({
    if (!scene || !camera || !params || (!out_device && !film)) return RAYRS_INVALID_ARG;
    if (scene->device < 0) return RAYRS_NO_DEVICE;
    if (params->spp == 0 || camera->x_pixels == 0 || camera->y_pixels == 0) return RAYRS_INVALID_ARG;
    if (camera->x_pixels > 65535u || camera->y_pixels > 65535u) return RAYRS_UNSUPPORTED;  // TailSlot::pix is 16 + 16 bits
    // a path's bounce count and RNG draw index travel as 16 bits each (15 + 16 in the local pool); a bounce draws at
    // most four numbers (material.rs:579 + :1009-1011 + lib.rs:539), so 8000 bounces stay below 2^15 and 2^16
    if (params->max_bounces > 8000u) return RAYRS_UNSUPPORTED;
    if (params->spp > SLOT_SAMPLE_MASK || sample0 > SLOT_SAMPLE_MASK - params->spp) return RAYRS_UNSUPPORTED;  // a slot's sample cursor has 30 bits
    if (params->tile_ranks == 0 || params->tile_rank >= params->tile_ranks) return RAYRS_INVALID_ARG;
    if (params->out_format != RAYRS_OUT_F32 && params->out_format != RAYRS_OUT_F64) return RAYRS_INVALID_ARG;
    if (params->fast_traversal > 1u) return RAYRS_INVALID_ARG;
    HIP_TRY(hipSetDevice(scene->device));
    hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
    if (scene->pending) {  // one render in flight per scene: its counters and partial sums are shared
        HIP_TRY(hipStreamSynchronize(scene->last_stream));
        scene->pending = false;
    }

    FramePlan p;
    RAYRS_TRY(plan_frame(scene, camera, params, sample0, film, out_device, p));
    p.is_film = film != nullptr;
    p.film = film ? *film : FilmPassDev{};
    scene->last_exact = p.exact;

    // ---- what the plan needs of the scene's buffers, which only grow (nothing of the route the frame does not take)
    rayrs_scene::Pool& pl = scene->pool;
    HIP_TRY(scene->d_partial.reserve((size_t)p.partial_need * 3 * sizeof(double)));
    p.rp.partial = scene->d_partial.as<double>();
    HIP_TRY(scene->d_local_light.reserve((size_t)p.local_blocks * 4u * LP_PATHS_PER_WAVE * 4 * sizeof(double)));
    HIP_TRY(pl.block.reserve((size_t)p.np * POOL_SLOT_BYTES));
    HIP_TRY(pl.d_wave_items.reserve((size_t)p.flat_blocks * 4u * 2 * sizeof(unsigned long long)));
    HIP_TRY(pl.d_stack_spill.reserve(p.spill_words * sizeof(uint32_t)));
    WfDev wf = pool_wf(pl.block, p.np, pl.d_ctl, p.trav_blocks, pl.d_stack_spill);
    wf.n_flat_waves = p.flat_blocks * 4u;
    wf.wave_items = pl.d_wave_items.as<unsigned long long>();

    pl.timed_rounds = 0;
    HIP_TRY(hipMemsetAsync(p.rp.counters, 0, sizeof(Counters), stream));
    HIP_TRY(hipMemsetAsync(p.rp.next_item, 0, sizeof(unsigned long long), stream));
    if (p.use_local) HIP_TRY(hipMemsetAsync(scene->d_local_items.as<>(), 0, LOCAL_MAX_SEGMENTS * sizeof(unsigned long long), stream));
    HIP_TRY(hipEventRecord(scene->ev[0], stream));
    scene->rounds = 0;
    scene->last_local = p.use_local;
    if (p.rp.total_items > 0) RAYRS_TRY(p.use_local ? enqueue_local(scene, p, stream) : enqueue_streaming(scene, p, wf, stream));
    HIP_TRY(hipEventRecord(scene->ev[1], stream));
    if (!p.use_local) HIP_TRY(p.is_film ? launch_film_accumulate(p.cam, p.rp, p.film, 0u, p.rp.n_local_tiles, stream) : launch_resolve(p.cam, p.rp, 0u, p.rp.n_local_tiles, stream));
    HIP_TRY(hipEventRecord(scene->ev[2], stream));
    scene->last_stream = stream;
    scene->pending = true;
    return RAYRS_OK;
    })
}

int rayrs_render_launch(rayrs_scene* scene, const rayrs_camera* camera, const rayrs_render_params* params,
                        void* out_device, void* hip_stream) {
    if (!out_device) return RAYRS_INVALID_ARG;
    return render_enqueue(scene, camera, params, 0u, nullptr, out_device, hip_stream);
}

int rayrs_render_finish(rayrs_scene* scene, rayrs_render_stats* stats) {
    if (!scene) return RAYRS_INVALID_ARG;
    if (scene->device < 0) return RAYRS_NO_DEVICE;
    if (!scene->pending) return RAYRS_INVALID_ARG;
    HIP_TRY(hipSetDevice(scene->device));
    HIP_TRY(hipEventSynchronize(scene->ev[2]));
    scene->pending = false;
    if (stats) {
        Counters c;
        HIP_TRY(scene->d_counters.download(&c, sizeof(c)));
        std::memset(stats, 0, sizeof(*stats));
        stats->rays = c.rays;
        stats->paths = c.paths;
        stats->nan_pixels = c.nan_pixels;
        stats->neg_pixels = c.neg_pixels;
        stats->interior_visits = c.interior_visits;
        stats->tri_tests = c.tri_tests;
        stats->sphere_tests = c.sphere_tests;
        stats->plane_tests = c.plane_tests;
        stats->escaped_paths = c.escaped_paths;
        stats->step_wave = c.step_wave, stats->step_lane = c.step_lane, stats->inner_wave = c.inner_wave;
        stats->leaf_wave = c.leaf_wave, stats->interior_ticks = c.interior_ticks, stats->leaf_ticks = c.leaf_ticks;
        stats->refill_ticks = c.refill_ticks;
        for (int k = 0; k < 8; k++) stats->surface_hits[k] = c.surface_hits[k];
        stats->direct_rays = c.direct_rays;
        stats->pre_rays = c.pre_rays, stats->pre_root_records = c.pre_root_records, stats->hot_lane = c.hot_lane;
        stats->hot_prim_tests = c.hot_prim_tests, stats->hot_tri_divided = c.hot_tri_divided;
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, scene->ev[0], scene->ev[1]));
        stats->trace_ms = ms;
        HIP_TRY(hipEventElapsedTime(&ms, scene->ev[0], scene->ev[2]));
        stats->total_ms = ms;
        const uint32_t timed_rounds = scene->pool.timed_rounds;
        double t = 0.0, h = 0.0, m = 0.0;
        for (uint32_t r = 0; r < timed_rounds; r++) {
            float k[3];
            RAYRS_TRY(round_ms(scene, r, k));
            t += k[0], h += k[1], m += k[2];
        }
        // rounds beyond the event pool (very long renders) are extrapolated from the timed ones
        if (timed_rounds && scene->rounds > timed_rounds) {
            const double f = (double)scene->rounds / (double)timed_rounds;
            t *= f, h *= f, m *= f;
        }
        stats->kernel_ms = t;
        stats->hit_ms = h, stats->miss_ms = m;
        stats->local_pool = scene->last_local ? 1u : 0u;
        stats->exact_walk = (scene->last_exact || scene->last_local) ? 1u : 0u;
        stats->hot_group = (!scene->last_local && scene->last_exact && scene->walk_index(true) == 2) ? 1u : 0u;
        stats->kernel_launches = (uint64_t)scene->rounds;
    }
    return RAYRS_OK;
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
