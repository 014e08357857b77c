// radiance_lit.hip -- the radiance queries with light sampling (include/rayrs_hip.h LIGHT SAMPLING).  A unit of its own beside
// radiance.hip, whose wave it restates: one path per lane from its first ray to its last, in registers, fused with the
// closest-hit walk in its resumable pieces; finished lanes are shaded, idle lanes refilled from one device-wide cursor, one
// record or one leaf group per step.  What differs is the surface's evaluation (radiance_lit_device.h lit_material_evaluate, with
// the light list in the kernel arguments) and a third way for a sample to start, the camera's pixel.
#include <hip/hip_runtime.h>

#include "device_path.h"
#include "launch_dispatch.h"
#include "radiance_lit_device.h"
#include "radiance_lit_kernels.h"
#include "radiance_wave_parts.h"

namespace rayrs {

// The start of sample s of ray (point, pixel) `ray`: its RNG and its first ray; `first` is what the sample's value is multiplied
// by at its end (LIT_START_POINT with lights: the colour of the operation at the point; read by no other start).
struct LitStart {
    Rng rng;
    V3 o, d, first;
};
template <int START>
RR_DEV LitStart lit_sample_start(const RadianceDev& rd, const LightsDev& lights, const CameraDev& cam, uint32_t ray, uint32_t s) {
    SampleStart st = sample_start(QueryStart<START>{}, rd, cam, ray, s);
    V3 first = mk(1.0, 1.0, 1.0);
    if (START == LIT_START_POINT) {
        const V3 n = st.d;
        if (lights.n != 0u) {
            const Scatter ev = lit_lambertian_scatter(mk(1.0, 1.0, 1.0), st.o, n, st.rng, lights);
            st.d = ev.dir, first = ev.color;
        } else {  // IRRADIANCE's ray
            st.d = cosine_direction(n, st.rng);
        }
    }
    return LitStart{st.rng, st.o, st.d, first};
}

// radiance.hip radiance_kernel's wave and its termination argument, turn for turn; a chunk's sum is made in this one lane in
// sample order and stored once, so no f64 sum depends on which lanes did what when.
template <bool COMPACT, bool EXACT, int START>
__global__ void __launch_bounds__(256) radiance_lit_kernel(SceneDev sc, RadianceDev rd, LightsDev lights, CameraDev cam) {
    extern __shared__ uint32_t lds_stack[];
    const LaneStack stack = lane_stack(lds_stack, rd.spill, sc);
    const unsigned long long n_items = (unsigned long long)rd.n * rd.chunks;

    bool has = false;  // the lane holds a path: walking while tv.cur != TRAV_DONE, then finished (waiting to be shaded)
    uint32_t item = 0, ray = 0;
    uint32_t s = 0, s_end = 0;  // the path's sample, the chunk's end
    uint32_t bounce = 0, queries = 0;
    Rng rng{0, 0};
    V3 o = mk(0, 0, 0), d = mk(0, 0, 1);
    V3 thr = mk(1, 1, 1), light = mk(0, 0, 0), sum = mk(0, 0, 0), first = mk(1, 1, 1);
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
            // ---- shade: one turn of radiance()'s loop for every finished lane (lib.rs:526-556), evaluate with Some(pdf)
            if (do_shade && fin) {
                bool ended = true;
                V3 result;
                if (tv.best_prim != 0xffffffffu) {
                    const PrimRec<COMPACT> rec = load_prim<COMPACT>(sc.prims, tv.best_prim);
                    const V3 position = hit_position(o, d, tv.best_t);
                    const HitPoint hp = hit_point<COMPACT>(rec, position, d);
                    const SurfaceDev* surf = sc.surfaces + hp.sid;
                    const Scatter ev = lit_material_evaluate(surf, position, hp.normal, hp.view, rng, lights);
                    const bool goes_on = ev.scatter && bounce_step(ev.color, surf->emit, rng.next(), bounce + 1u, NO_BOUNCE_BOUND, thr, light);
                    bounce++;
                    result = light;  // lib.rs:550, the roulette, or lib.rs:559
                    if (goes_on && bounce < rd.max_bounces) o = position, d = ev.dir, ended = false, new_ray = true;
                } else {
                    result = escape(sc, d, thr, light);
                }
                if (ended) {
                    if (START == LIT_START_POINT && lights.n != 0u) result = v_mul(first, result);
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
                const LitStart st = lit_sample_start<START>(rd, lights, cam, ray, s);
                rng = st.rng, o = st.o, d = st.d;
                if (START == LIT_START_POINT) first = st.first;
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
            if (at_leaf) closest_leaf_step<COMPACT>(sc, o, d, stack, tv);
        } else {
            if (at_int) closest_interior_step<COMPACT, EXACT>(sc, o, stack, tv);
        }
    }
}

__global__ void __launch_bounds__(256) radiance_lit_resolve_kernel(RadianceDev rd) { radiance_resolve(rd); }

hipError_t launch_radiance_lit(bool compact, const SceneDev& sc, const RadianceDev& rd, const LightsDev& lights, const CameraDev& cam,
                               int start, int cu_count, hipStream_t stream) {
    if (rd.n == 0u) return hipSuccess;
    const hipError_t e = with_lit_start([&](auto S) {
        return with_bools([&](auto C, auto E) {
            return launch_lane_stacks(&radiance_lit_kernel<decltype(C)::value, decltype(E)::value, decltype(S)::value>,
                                      radiance_grid_blocks(rd, cu_count), sc.stack_lds, stream, sc, rd, lights, cam);
        }, compact, sc.exact != 0u);
    }, start);
    if (e != hipSuccess) return e;
    return launch_radiance_resolve(radiance_lit_resolve_kernel, rd, stream);
}

}  // namespace rayrs
