// scene_device.cpp -- a scene on its device: the upload, the traversal kernel's LDS sizing per tree, the local-pool route's
// gating boxes, what a render hands its kernels of the scene (SceneDev), and the handle's end.
#include <hip/hip_runtime.h>

#include <cstring>

#include "local_pool.h"
#include "scene_host.hpp"
#include "scene_internal.hpp"
#include "wavefront.h"

using namespace rayrs;

namespace {
constexpr uint32_t TRAV_STACK_LDS = 12;
constexpr uint32_t TRAV_HOT_BYTES = 14u * 1024u;
// The trees the default walk reads: a lane's leaf groups wait in a queue of LEAFQ entries behind its stack
// (device_path.h trav_interior_step_defer), so its stack holds interior records only -- 8 entries in LDS serve what 12
// served with the leaves among them -- and the records kept in LDS give up the other 4 KiB of the queue's 8.
constexpr uint32_t TRAV_STACK_LDS_DEFER = 8;
constexpr uint32_t TRAV_HOT_BYTES_DEFER = 10u * 1024u;
}  // namespace

// A render in flight ends before any member releases what it uses (nothing here touches rayrs_last_error).
rayrs_scene::~rayrs_scene() {
    if (device < 0) return;
    (void)hipSetDevice(device);
    (void)frame.wait();
}

namespace rayrs {

// Sizes the traversal workgroup's LDS from the tree and the scene's tuning, and asks the runtime how
// many such workgroups fit a CU.  A workgroup's LDS: the first stack_lds entries of each lane's stack
// (deeper entries overflow to HBM; on the 1M-triangle scene 99.4 % of visits happen with at most 7
// pending), 4 KiB of window lists, and the hot_records largest wide records.  13 + 4 + 14 KiB (the default walk's trees: 17 KiB with the lanes' leaf queues + 4 + 10) lets
// five workgroups (the kernel's launch bound) share a CU's 160 KiB.
// The kernel's dynamic-LDS limit belongs to the kernel on a device, not to a scene, and the scenes of a process share
// it: it is only ever raised (wf_trav_raise_lds), so it ends at no less than the largest size among the trees this scene has.
int scene_configure_traversal(rayrs_scene* s) {
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
void scene_configure_local(rayrs_scene* s) {
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

int scene_upload(rayrs_scene* s) {
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
    HIP_TRY(s->frame.d_counters.reserve(sizeof(Counters)));
    for (auto& e : s->frame.ev) HIP_TRY(e.create());
    s->device_bytes = f.walk.node_bytes.size() + f.gate.node_bytes.size() + (f.has_hot ? f.gate_hot.node_bytes.size() : 0) + f.prim_bytes.size() + s->surfaces.size() * sizeof(SurfaceDev) +
                      f.hdri_quads.size() * sizeof(float);
    RAYRS_TRY(scene_configure_traversal(s));
    HIP_TRY(s->frame.pool.d_ctl.reserve(sizeof(WfCtl)));
    HIP_TRY(s->frame.pool.h_live.alloc(2 * sizeof(uint32_t)));
    for (auto& e : s->frame.pool.ev_batch) HIP_TRY(e.create());
    HIP_TRY(s->frame.d_next_item.reserve(sizeof(unsigned long long)));
    if (s->local_ok) {
        HIP_TRY(lp_configure());
        // (from about 13 primitives and surface rows up three workgroups' LDS no longer fit a CU: ask, do not assume)
        HIP_TRY(lp_occupancy(s->flat.compact, s->local.n_prims, (uint32_t)s->surfaces.size(), &s->local_blocks_per_cu));
        if (s->local_blocks_per_cu < 1) s->local_blocks_per_cu = 1;
        if (s->local_blocks_per_cu > (int)LP_WPS) s->local_blocks_per_cu = (int)LP_WPS;
        HIP_TRY(s->frame.d_local_items.reserve(LOCAL_MAX_SEGMENTS * sizeof(unsigned long long)));
    }
    return RAYRS_OK;
}

// Only the ray queries map a depth-first slot to its object on the device (a render's host side does it after the
// download), so the table goes up with the first of them and stays.
int scene_prim_object(rayrs_scene* s, const uint32_t** out) {
    rayrs_scene::Queries& q = s->queries;
    if (!q.has_prim_object) {
        const std::vector<uint32_t>& prim_object = s->flat.prim_object;
        HIP_TRY(q.d_prim_object.upload(prim_object.data(), prim_object.size() * sizeof(uint32_t)));
        q.has_prim_object = true;
    }
    *out = q.d_prim_object.as<uint32_t>();
    return RAYRS_OK;
}

SceneDev make_scene_dev(const rayrs_scene* s, bool exact) {
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
    sc.stack_depth = s->stack_depth(which);
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

}  // namespace rayrs
