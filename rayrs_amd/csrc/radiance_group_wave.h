// radiance_group_wave.h -- the wave of the radiance queries with a mesh-light group among the lights of direct lighting, written
// once for both ways of drawing from the group (GROUP: MeshDev, include/rayrs_hip.h MESH LIGHTS, by area; TreeDev, LIGHT TREE, by
// the tree's descent from the shading point) and for whoever starts its paths: the queries (radiance_mesh.hip, radiance_tree.hip),
// the film's and the bake's passes (film_mesh.hip, bake_mesh.hip) and the probes (radiance_probe.hip).  It is
// radiance_direct_wave.h's wave restated with the group's bounce -- one path per lane, two rays per diffuse bounce, the same state
// between them -- and what differs is this: every diffuse bounce has a shadow sample (the group is never empty here), its direction
// may come from the group's tables, a shadow ray aimed at a triangle is credited only where that very triangle is its closest
// hit, and a listed triangle met by the path's own ray is weighted in area measure at the hit.  So a lane carries three more words
// than the direct wave's: pc of its last diffuse bounce, and the slot its shadow ray was aimed at.  What the two groups do
// differently is behind four overloads of radiance_mesh_device.h and radiance_tree_device.h: group_bounce, and group_met,
// group_listed and group_met_weight for a primitive the path's own ray met (the area group tells it from one bitmap word; the
// tree from one word of its entry table, which is the entry whose path the met weight descends).
#pragma once
#include "device_path.h"
#include "radiance_direct_wave.h"
#include "radiance_mesh_device.h"
#include "radiance_mesh_kernels.h"
#include "radiance_tree_device.h"

namespace rayrs {

// The start of sample s of ray (point, pixel) `ray`: its RNG and its first ray.  LIT_START_POINT is IRRADIANCE, DIRECT's virtual
// bounce, whatever K is: `first` is its shadow sample and the weights of what the first ray meets.
struct MeshStart {
    Rng rng;
    V3 o, d;
    MeshBounce first;
};
template <bool SKY, class START, class GROUP>
RR_DEV MeshStart group_path_start(const START& start, const RadianceDev& rd, const LightsDev& lights, const GROUP& group, const SkyDev& sky,
                                  const CameraDev& cam, uint32_t ray, uint32_t s) {
    SampleStart st = sample_start(start, rd, cam, ray, s);
    MeshBounce first;
    first.shadow = false, first.l_s = mk(0.0, 0.0, 1.0), first.credit = mk(0.0, 0.0, 0.0), first.w_next = 1.0, first.pc = 0.0;
    first.aim = MESH_NO_AIM;
    if (START::KIND == LIT_START_POINT) {  // IRRADIANCE's ray, then the virtual bounce at the point, whatever K is
        const V3 n = st.d;
        st.d = cosine_direction(n, st.rng);
        first = group_bounce<SKY>(mk(1.0, 1.0, 1.0), mk(1.0, 1.0, 1.0), st.o, n, st.d, st.rng, lights, group, sky);
    }
    return MeshStart{st.rng, st.o, st.d, first};
}

// radiance_direct_wave.h direct_wave's wave and its termination argument, turn for turn: a lane that holds a path either walks
// (its path's ray or a shadow ray) or waits to be shaded, every shade turn ends a ray, and a path has at most
// 2 * max_bounces + 1 of them.  A chunk's sum is made in this one lane in sample order and stored once, so no f64 sum depends on
// which lanes did what when.  The group's tables are read inside group_bounce and group_met_weight (by indices the area group's
// search keeps inside them, by references the tree's build wrote, which stay inside them whatever the point is) and, one word of
// the bitmap or of the entry table, at a hit (by the slot of a primitive the walk answered with).
template <bool COMPACT, bool EXACT, bool SKY, class START, class GROUP>
RR_DEV void group_wave(const START& start, const LaneStack& stack, const SceneDev& sc, const RadianceDev& rd, const LightsDev& lights,
                       const LightSlotsDev& slots, const GROUP& group, const SkyDev& sky, const CameraDev& cam) {
    constexpr bool POINT = START::KIND == LIT_START_POINT;
    const unsigned long long n_items = start.n_items(rd);
    const double m_lights = (double)(lights.n + 1u + (SKY ? 1u : 0u));  // (double)M

    bool has = false;  // the lane holds a path: walking while tv.cur != TRAV_DONE, then finished (waiting to be shaded)
    uint32_t item = 0, ray = 0;
    uint32_t s = 0, s_end = 0;  // the path's sample, the chunk's end
    uint32_t bounce = 0, queries = 0;
    Rng rng{0, 0};
    V3 o = mk(0, 0, 0), d = mk(0, 0, 1);
    V3 thr = mk(1, 1, 1), light = mk(0, 0, 0), sum = mk(0, 0, 0);
    V3 first = mk(0, 0, 0);  // LIT_START_POINT: the virtual bounce's credit, added to the path's value at its end
    // the ray the lane walks is a shadow ray; after it the path goes on along l (else the sample ends); the shadow sample's worth
    bool shadow = false, goes_on = false;
    V3 l = mk(0, 0, 1), credit = mk(0, 0, 0);
    uint32_t aim = MESH_NO_AIM;  // the slot of the triangle the shadow ray was aimed at, if the group was drawn
    double w = 1.0;    // the weight of a listed lamp's emission, or the sky's, met by the path's ray
    double pc = 0.0;   // the cosine arm's density of the path's ray, which weights a listed triangle it meets ...
    bool lit = false;  // ... where the ray left a diffuse bounce (else that weight is 1.0)
    Trav tv;
    tv.inv = mk(0, 0, 0), tv.best_t = 0, tv.best_prim = 0xffffffffu, tv.cur = TRAV_DONE, tv.sp = 0;
    bool no_more = false;  // wave-uniform: the cursor ran off the launch's items

    for (;;) {
        const bool live = has && tv.cur != TRAV_DONE;
        const bool at_int = live && trav_at_interior(tv);
        const bool at_leaf = live && !trav_at_interior(tv);
        const bool fin = has && tv.cur == TRAV_DONE;
        const int n_int = __popcll(__ballot(at_int));
        const int n_leaf = __popcll(__ballot(at_leaf));
        const int n_fin = __popcll(__ballot(fin));
        const int n_walk = n_int + n_leaf;
        const bool do_shade = n_fin > 0 && (n_fin >= (int)rd.shade_at || n_walk == 0);
        const bool do_refill = !no_more && n_walk < (int)rd.refill_below && (do_shade || n_walk + n_fin < 64);
        if (do_shade || do_refill) {
            bool new_sample = false, new_ray = false;
            // ---- shade: for every finished lane, the end of its shadow ray or one turn of radiance()'s loop (lib.rs:526-556)
            if (do_shade && fin) {
                bool ended = true;
                V3 result = light;
                if (shadow) {  // the shadow sample's credit, then the continuation or the sample's end (the roulette's word)
                    const bool missed = tv.best_prim == 0xffffffffu;
                    // aimed at a triangle: that triangle alone earns; else the sky's light (SKY), or a listed lamp's
                    const bool earns = aim != MESH_NO_AIM ? tv.best_prim == aim
                                                          : missed ? SKY : direct_listed(lights, slots, tv.best_prim);
                    if (earns) {
                        V3 source;
                        if (SKY && missed) {
                            source = background(sc, d);
                        } else {
                            const PrimRec<COMPACT> rec = load_prim<COMPACT>(sc.prims, tv.best_prim);
                            const double* emit = sc.surfaces[rec.tag() >> 8].emit;
                            source = mk(emit[0], emit[1], emit[2]);
                        }
                        const V3 worth = v_mul(credit, source);
                        if (POINT && bounce == 0u) first = worth;  // (the path has not met a surface yet)
                        else light = v_add(light, worth);
                    }
                    shadow = false;
                    result = light;
                    if (goes_on) d = l, ended = false, new_ray = true;
                } else if (tv.best_prim != 0xffffffffu) {
                    const PrimRec<COMPACT> rec = load_prim<COMPACT>(sc.prims, tv.best_prim);
                    const V3 position = hit_position(o, d, tv.best_t);
                    const HitPoint hp = hit_point<COMPACT>(rec, position, d);
                    const SurfaceDev* surf = sc.surfaces + hp.sid;
                    bool diffuse;
                    const Scatter ev = direct_material_evaluate(surf, hp.normal, hp.view, rng, diffuse);
                    if (ev.scatter) {
                        V3 e = mk(surf->emit[0], surf->emit[1], surf->emit[2]);
                        const auto met = group_met(group, tv.best_prim);  // a listed triangle: which one, where the group asks
                        if (group_listed(group, met)) {
                            if (lit) e = v_scale(e, group_met_weight(group, met, m_lights, pc, o, d, position, hp.normal));
                        } else if (direct_listed(lights, slots, tv.best_prim)) {
                            e = v_scale(e, w);
                        }
                        light = v_add(light, v_mul(thr, e));
                        w = 1.0, lit = false;
                        if (diffuse) {
                            const MeshBounce mb = group_bounce<SKY>(mk(surf->color[0], surf->color[1], surf->color[2]), thr, position,
                                                                    hp.normal, ev.dir, rng, lights, group, sky);
                            shadow = mb.shadow, credit = mb.credit, w = mb.w_next, pc = mb.pc, aim = mb.aim, lit = true;
                            if (shadow) d = mb.l_s;
                        }
                        thr = v_mul(thr, ev.color);  // the roulette and DivAssign (device_path.h bounce_step)
                        const double p = rr_max(rr_max(thr.x, thr.y), thr.z);
                        goes_on = !(rng.next() > p);
                        if (goes_on) thr = mk(thr.x / p, thr.y / p, thr.z / p);
                        bounce++;
                        goes_on = goes_on && bounce < rd.max_bounces;
                        result = light;  // lib.rs:550, the roulette, or lib.rs:559
                        if (shadow) o = position, l = ev.dir, ended = false, new_ray = true;
                        else if (goes_on) o = position, d = ev.dir, ended = false, new_ray = true;
                    }
                } else if (SKY) {
                    result = v_add(light, v_mul(thr, v_scale(background(sc, d), w)));  // light + throughput * (background(dir) * w)
                } else {
                    result = escape(sc, d, thr, light);
                }
                if (ended) {
                    if (POINT) result = v_add(first, result);  // L = credit + radiance(..)
                    sum = v_add(sum, result);
                    s++;
                    if (s < s_end) {
                        new_sample = true;
                    } else {  // the chunk is done: plain vector stores, and the lane is idle
                        double* dst = rd.partial + (size_t)item * 3u;
                        dst[0] = sum.x, dst[1] = sum.y, dst[2] = sum.z;
                        rd.partial_queries[item] = queries;
                        has = false;
                    }
                }
            }
            // ---- refill: idle lanes take the next items, lowest lane first (a start that SKIPS: direct_wave's rule)
            if (do_refill) {
                for (;;) {
                    bool need = !has;
                    const unsigned long long need_mask = __ballot(need);
                    if (need_mask == 0ull) break;
                    const uint32_t wanted = (uint32_t)__popcll(need_mask);
                    unsigned long long base = 0ull;
                    if ((threadIdx.x & 63u) == 0u) base = atomicAdd(rd.cursor, (unsigned long long)wanted);
                    base = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32)) << 32) |
                           (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
                    const unsigned long long left = base < n_items ? n_items - base : 0ull;
                    const uint32_t avail = left < wanted ? (uint32_t)left : wanted;
                    if (need && lanes_below(need_mask) < avail) {
                        item = (uint32_t)base + lanes_below(need_mask);  // (n_items <= 2^20)
                        if (start.take(rd, cam, item, ray, s, s_end)) {
                            sum = mk(0.0, 0.0, 0.0);  // C_k = Vec3::zeros()
                            queries = 0u;
                            has = true, new_sample = true;
                        }
                    }
                    if (avail < wanted) no_more = true;
                    if (!START::SKIPS || no_more) break;
                }
            }
            // ---- a new sample's start; every new ray is one Bvh::intersect call
            if (new_sample) {
                const MeshStart st = group_path_start<SKY>(start, rd, lights, group, sky, cam, ray, s);
                rng = st.rng, o = st.o, d = st.d;
                thr = mk(1.0, 1.0, 1.0), light = mk(0.0, 0.0, 0.0);
                bounce = 0u;
                shadow = false, w = 1.0, lit = false;
                if (POINT) first = mk(0.0, 0.0, 0.0);
                if (POINT) {  // the virtual bounce: no roulette, the path goes on (max_bounces >= 1)
                    shadow = st.first.shadow, credit = st.first.credit, w = st.first.w_next, pc = st.first.pc, aim = st.first.aim;
                    lit = true, goes_on = true;
                    if (shadow) l = d, d = st.first.l_s;
                }
                new_ray = true;
            }
            if (new_ray) {
                trav_init(sc, o, d, tv);
                queries++;
            }
            // ---- the whole wave: fresh lanes get the hot group's test, where the scene has one, before they walk
            closest_start<EXACT>(sc, o, d, new_ray, tv);
            continue;
        }
        if (n_walk == 0) break;  // (no lane holds a path and no item is left)
        const bool leaf_phase = n_leaf >= (int)rd.leaf_min || n_int == 0;
        if (leaf_phase) {
            if (at_leaf) closest_leaf_step<COMPACT>(sc, o, d, stack, tv);
        } else {
            if (at_int) closest_interior_step<COMPACT, EXACT>(sc, o, stack, tv);
        }
    }
}

}  // namespace rayrs
