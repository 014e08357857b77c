// radiance.hip -- radiance queries (include/rayrs_hip.h RADIANCE QUERY, IRRADIANCE).  The kernels are not part of a render
// and a unit of their own, as query.hip's and ao.hip's: the radiance loop of device_path.h runs fused with the closest-hit
// walk in its resumable pieces, one path per lane from its first ray to its last, in registers.  A lane whose path ends takes
// the chunk's next sample or the next (ray, chunk) item instead of waiting for the wave's longest path.
#include <hip/hip_runtime.h>

#include "device_path.h"
#include "launch_dispatch.h"
#include "radiance_kernels.h"
#include "radiance_wave_parts.h"

namespace rayrs {

// The start of sample s of ray (point) `ray`: its RNG and its first ray.  RADIANCE QUERY: the caller's ray, draw 0 next.
// IRRADIANCE: AMBIENT OCCLUSION's ray (ao.hip ao_ray: device_path.h cosine_direction) on draws 0 and 1, draw 2 next.
template <bool IRRADIANCE>
RR_DEV void radiance_sample_start(const RadianceDev& rd, uint32_t ray, uint32_t s, Rng& rng, V3& o, V3& d) {
    const double* pa = rd.a + (size_t)ray * 3u;
    const double* pb = rd.b + (size_t)ray * 3u;
    const V3 a = mk(pa[0], pa[1], pa[2]), b = mk(pb[0], pb[1], pb[2]);
    rng = Rng{rr_path_key(rd.seed, rd.index_base + ray, (uint64_t)s), 0};
    if (IRRADIANCE) {
        d = cosine_direction(b, rng);
        o = v_add(a, v_scale(b, rd.bias));
    } else {
        o = a, d = b;
    }
}

// The grid's waves take items from rd.cursor.  A lane holds one path of its item's chunk at a time: the ray, throughput and
// light, the RNG, the bounce number, the sample cursor, the chunk's sum, its query count and a resumable Trav.  A chunk's sum
// is made in this one lane in sample order and stored once, so no f64 sum depends on which lanes did what when.  IRRADIANCE:
// the items are (point, chunk) and a sample's first ray is made here.  STEPS: the lab's instance, which also counts turns
// (never timed).
template <bool COMPACT, bool EXACT, bool IRRADIANCE, bool STEPS>
__global__ void __launch_bounds__(256) radiance_kernel(SceneDev sc, RadianceDev rd) {
    extern __shared__ uint32_t lds_stack[];
    const LaneStack stack = lane_stack(lds_stack, rd.spill, sc);
    const unsigned long long n_items = (unsigned long long)rd.n * rd.chunks;

    bool has = false;  // the lane holds a path: walking while tv.cur != TRAV_DONE, then finished (waiting to be shaded)
    uint32_t item = 0, ray = 0;
    uint32_t s = 0, s_end = 0;  // the path's sample, the chunk's end
    uint32_t bounce = 0, queries = 0;
    Rng rng{0, 0};
    V3 o = mk(0, 0, 0), d = mk(0, 0, 1);
    V3 thr = mk(1, 1, 1), light = mk(0, 0, 0), sum = mk(0, 0, 0);
    Trav tv;
    tv.inv = mk(0, 0, 0), tv.best_t = 0, tv.best_prim = 0xffffffffu, tv.cur = TRAV_DONE, tv.sp = 0;
    bool no_more = false;  // wave-uniform: the cursor ran off the launch's items
    uint32_t wave_turns = 0, walk_turns = 0, shade_turns = 0;

    // Termination.  A turn is a service turn (shade and / or refill), a step turn, or the last.
    //  - A service turn is taken when it shades (do_shade: some lane is finished) or refills with a lane to fill (do_refill
    //    without do_shade: items may be left and some lane is idle).  Shading a finished lane either gives its path the next
    //    ray -- the bounce number grows, and a path ends at max_bounces at the latest -- or ends the path, which moves the
    //    item's sample cursor forward -- an item has at most `chunk` samples -- or retires the item.  A refill with an idle
    //    lane moves the cursor forward by the number of idle lanes (>= 1); the cursor is only ever added to, so after finitely
    //    many refills it is at or past n_items, no_more is set and do_refill is false for good.  Either way something that
    //    is bounded has advanced; a service turn that does neither is never taken.
    //  - Otherwise, with no lane walking there is no lane finished either (do_shade would hold: it needs no threshold when
    //    none walks), so all 64 are idle, and since do_refill is false with n_walk = 0 < refill_below, no_more is set: the
    //    wave leaves, with nothing in flight and every item it took stored.
    //  - Otherwise a step turn: at least one lane walks, and the phase it runs has at least one lane in it (a leaf phase
    //    needs leaf_min >= 1 lanes there or no lane at a record; else some lane is at a record): that lane's walk advances by
    //    one record or one leaf group, and a walk is finite.
    // So every turn retires, refills, shades or advances at least one lane, and none of these can recur for ever.
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
        if (STEPS) wave_turns++;
        if (do_shade || do_refill) {
            bool new_sample = false, new_ray = false;
            // ---- shade: one turn of radiance()'s loop for every finished lane (lib.rs:526-556)
            if (do_shade && fin) {
                if (STEPS) shade_turns++;
                bool ended = true;
                V3 result;
                if (tv.best_prim != 0xffffffffu) {
                    const PrimRec<COMPACT> rec = load_prim<COMPACT>(sc.prims, tv.best_prim);
                    const V3 position = hit_position(o, d, tv.best_t);
                    const HitPoint hp = hit_point<COMPACT>(rec, position, d);
                    const SurfaceDev* surf = sc.surfaces + hp.sid;
                    const Scatter ev = material_evaluate(surf, hp.normal, hp.view, rng);
                    // (the loop's bound is this kernel's, as in kernels.hip test_path_trace_kernel: the bounce is told of none)
                    const bool goes_on = ev.scatter && bounce_step(ev.color, surf->emit, rng.next(), bounce + 1u, NO_BOUNCE_BOUND, thr, light);
                    bounce++;
                    result = light;  // lib.rs:550, the roulette, or lib.rs:559
                    if (goes_on && bounce < rd.max_bounces) o = position, d = ev.dir, ended = false, new_ray = true;
                } else {
                    result = escape(sc, d, thr, light);
                }
                if (ended) {
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
            // ---- refill: idle lanes take the next items, lowest lane first
            if (do_refill) {
                bool need = !has;
                const unsigned long long need_mask = __ballot(need);
                if (need_mask != 0ull) {
                    const uint32_t wanted = (uint32_t)__popcll(need_mask);
                    unsigned long long base = 0ull;
                    if ((threadIdx.x & 63u) == 0u) base = atomicAdd(rd.cursor, (unsigned long long)wanted);
                    base = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32)) << 32) |
                           (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
                    const unsigned long long left = base < n_items ? n_items - base : 0ull;
                    const uint32_t avail = left < wanted ? (uint32_t)left : wanted;
                    if (need && lanes_below(need_mask) < avail) {
                        item = (uint32_t)base + lanes_below(need_mask);  // (n_items <= 2^20)
                        // (radiance_wave_parts.h QueryStart::take, written out: called, it moves these kernels' code)
                        ray = item / rd.chunks;
                        s = (item - ray * rd.chunks) * rd.chunk;
                        s_end = rd.samples - s < rd.chunk ? rd.samples : s + rd.chunk;
                        sum = mk(0.0, 0.0, 0.0);  // C_k = Vec3::zeros()
                        queries = 0u;
                        has = true, new_sample = true;
                    }
                    if (avail < wanted) no_more = true;
                }
            }
            // ---- a new sample's start; every new ray is one Bvh::intersect call
            if (new_sample) {
                radiance_sample_start<IRRADIANCE>(rd, ray, s, rng, o, d);
                thr = mk(1.0, 1.0, 1.0), light = mk(0.0, 0.0, 0.0);
                bounce = 0u;
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
            if (at_leaf) {
                if (STEPS) walk_turns++;
                closest_leaf_step<COMPACT>(sc, o, d, stack, tv);
            }
        } else {
            if (at_int) {
                if (STEPS) walk_turns++;
                closest_interior_step<COMPACT, EXACT>(sc, o, stack, tv);
            }
        }
    }

    if (STEPS) {
        atomicAdd(&rd.turns[1], (unsigned long long)walk_turns);
        atomicAdd(&rd.turns[2], (unsigned long long)shade_turns);
        if ((threadIdx.x & 63u) == 0u) atomicAdd(&rd.turns[0], 64ull * wave_turns);
    }
}

__global__ void __launch_bounds__(256) radiance_resolve_kernel(RadianceDev rd) { radiance_resolve(rd); }

hipError_t launch_radiance(bool compact, const SceneDev& sc, const RadianceDev& rd, int cu_count, hipStream_t stream) {
    if (rd.n == 0u) return hipSuccess;
    const hipError_t e = with_bools([&](auto C, auto E, auto I, auto S) {
        return launch_lane_stacks(&radiance_kernel<decltype(C)::value, decltype(E)::value, decltype(I)::value, decltype(S)::value>,
                                  radiance_grid_blocks(rd, cu_count), sc.stack_lds, stream, sc, rd);
    }, compact, sc.exact != 0u, rd.irradiance != 0u, rd.turns != nullptr);
    if (e != hipSuccess) return e;
    return launch_radiance_resolve(radiance_resolve_kernel, rd, stream);
}

}  // namespace rayrs
