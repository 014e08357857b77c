// ao.hip -- ambient occlusion (include/rayrs_hip.h AMBIENT OCCLUSION).  The kernels are not part of a render and a unit of
// their own, as query.hip's: the rays are made here, from the counter RNG and the cosine lobe as lambertian_scatter forms
// it, and answered by the any-hit walk of device_path.h in its resumable pieces, so that a lane whose ray is answered takes
// the next (point, sample) item instead of waiting for the wave's slowest ray.
#include <hip/hip_runtime.h>

#include "ao_kernels.h"
#include "device_path.h"
#include "launch_dispatch.h"

namespace rayrs {

// Sample s of point i: the operation of the header, its direction device_path.h cosine_direction's on draws 0 and 1.
RR_DEV void ao_ray(const AoDev& ao, uint32_t i, uint32_t s, V3& o, V3& l) {
    const double* pp = ao.position + (size_t)i * 3u;
    const double* pn = ao.normal + (size_t)i * 3u;
    const V3 p = mk(pp[0], pp[1], pp[2]), n = mk(pn[0], pn[1], pn[2]);
    Rng rng{rr_path_key(ao.seed, ao.index_base + i, (uint64_t)s), 0};
    l = cosine_direction(n, rng);
    o = v_add(p, v_scale(n, ao.bias));
}

// A workgroup owns the points blockIdx.x * block_points .. and their block_points x samples items, item k = (point k / samples,
// sample k % samples).  Its four waves take items from one cursor in LDS; a point's counter lives in LDS and is added to by
// whichever lanes answered its samples.  The count is an integer, so it is the same under any schedule; the stores at the
// end are plain vector stores, one thread per point.  STEPS: the lab's instance, which also counts turns (never timed).
template <bool COMPACT, bool EXACT, bool STEPS>
__global__ void __launch_bounds__(256) ao_kernel(SceneDev sc, AoDev ao) {
    extern __shared__ uint32_t lds_stack[];
    __shared__ uint32_t counts[AO_BLOCK_POINTS];
    __shared__ unsigned long long cursor;
    const LaneStack stack = lane_stack(lds_stack, ao.spill, sc);
    const uint32_t first = blockIdx.x * ao.block_points;  // (the grid covers n: first < n)
    const uint32_t n_points = ao.n - first < ao.block_points ? ao.n - first : ao.block_points;
    const unsigned long long n_items = (unsigned long long)n_points * ao.samples;
    if (threadIdx.x < AO_BLOCK_POINTS) counts[threadIdx.x] = 0u;
    if (threadIdx.x == 0u) cursor = 0ull;
    __syncthreads();

    bool walking = false, pending = false;  // pending: the lane holds an answered ray whose verdict is not in its counter yet
    uint32_t point = 0;                     // of the block
    V3 o = mk(0, 0, 0), d = mk(0, 0, 1);
    Trav tv;
    tv.inv = mk(0, 0, 0), tv.best_t = 0, tv.best_prim = 0xffffffffu, tv.cur = TRAV_DONE, tv.sp = 0;
    bool no_more = false;  // wave-uniform: the cursor ran off the block's items
    uint32_t wave_turns = 0, lane_turns = 0;

    // Termination.  A turn takes one of two branches.  The refill branch is entered with items left (!no_more) or with no
    // lane walking; with no_more it is left through the break below, which is then reached with nothing in flight (retired
    // just above it).  Otherwise every pass of its inner loop moves the cursor forward by the number of idle lanes (>= 1: a
    // wave with 64 walking lanes never refills, refill_below <= 64), and the cursor is only ever added to, so after finitely
    // many passes it is at or past n_items and no_more is set.  A step turn is entered with at least one lane walking, and
    // the phase it runs has at least one lane in it (a leaf phase needs AO_LEAF_MIN >= 1 lanes there or no lane at a record;
    // else some lane is at a record): that lane's walk advances by one record or one leaf group, and a walk is finite.  So
    // every turn retires, refills or advances a lane, none of which can go on for ever.
    for (;;) {
        const bool at_int = walking && trav_at_interior(tv);
        const bool at_leaf = walking && !trav_at_interior(tv);
        const int n_int = __popcll(__ballot(at_int));
        const int n_leaf = __popcll(__ballot(at_leaf));
        const int n_walk = n_int + n_leaf;
        if ((n_walk < (int)ao.refill_below && !no_more) || n_walk == 0) {
            // ---- retire: each answered ray adds its verdict to its point's counter
            if (pending) {
                if (occluded_found(tv, ao.t_max)) atomicAdd(&counts[point], 1u);
                pending = false;
            }
            if (no_more) break;  // (n_walk == 0: nothing in flight)
            // ---- idle lanes take the next items, lowest lane first
            bool fresh = false;
            bool need = !walking;
            unsigned long long need_mask = __ballot(need);
            while (need_mask != 0ull) {
                const uint32_t wanted = (uint32_t)__popcll(need_mask);
                unsigned long long base = 0ull;
                if ((threadIdx.x & 63u) == 0u) base = atomicAdd(&cursor, (unsigned long long)wanted);
                base = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32)) << 32) |
                       (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
                const unsigned long long left = base < n_items ? n_items - base : 0ull;
                const uint32_t avail = left < wanted ? (uint32_t)left : wanted;
                const uint32_t rank = lanes_below(need_mask);
                if (need && rank < avail) {
                    const unsigned long long item = base + rank;
                    point = (uint32_t)(item / ao.samples);
                    const uint32_t s = (uint32_t)(item - (unsigned long long)point * ao.samples);
                    if (ao.active == nullptr || ao.active[first + point] != 0u) {
                        ao_ray(ao, first + point, s, o, d);
                        trav_init(sc, o, d, tv);
                        fresh = true, need = false;
                    }
                }
                if (avail < wanted) {
                    no_more = true;
                    break;
                }
                need_mask = __ballot(need);  // (lanes whose item was an inactive point's ask again)
            }
            // ---- fresh lanes get the hot group's test, where the scene has one, before they join
            occluded_start<EXACT>(sc, o, d, ao.t_max, fresh, tv);
            if (fresh) {
                if (tv.cur == TRAV_DONE) pending = true;  // missed the root box, or answered by the hot group
                else walking = true;
            }
            continue;
        }
        const bool leaf_phase = n_leaf >= (int)AO_LEAF_MIN || n_int == 0;
        if (STEPS) wave_turns++;
        if (leaf_phase) {
            if (at_leaf) {
                if (STEPS) lane_turns++;
                occluded_leaf_step<COMPACT>(sc, o, d, ao.t_max, stack, tv);
                if (tv.cur == TRAV_DONE) walking = false, pending = true;
            }
        } else {
            if (at_int) {
                if (STEPS) lane_turns++;
                occluded_interior_step<COMPACT>(sc, o, stack, tv);
                if (tv.cur == TRAV_DONE) walking = false, pending = true;
            }
        }
    }

    __syncthreads();
    if (threadIdx.x < n_points) {
        const uint32_t c = counts[threadIdx.x];
        if (ao.count != nullptr) ao.count[first + threadIdx.x] = c;
        if (ao.visibility != nullptr) ao.visibility[first + threadIdx.x] = (double)(ao.samples - c) / (double)ao.samples;
    }
    if (STEPS) {
        atomicAdd(&ao.turns[1], (unsigned long long)lane_turns);
        if ((threadIdx.x & 63u) == 0u) atomicAdd(&ao.turns[0], 64ull * wave_turns);
    }
}

// The image form's first pass (AMBIENT OCCLUSION PLANE): features.hip's mapping, sample 0 only.  The lanes of an edge
// tile's padding trace the nearest pixel of the image beside them and store nothing.
template <bool COMPACT>
__global__ void __launch_bounds__(256) ao_primary_kernel(SceneDev sc, CameraDev cam, AoPrimaryDev pd) {
    extern __shared__ uint32_t lds_stack[];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6);
    const LaneStack stack = lane_stack(lds_stack, pd.spill, sc);
    if (wave >= pd.n_tiles) return;  // (wave-uniform)
    const TilePixel px = tile_pixel(pd.share, pd.tile0 + wave, lane);
    if (!px.in_share) return;
    const bool inside = px.row < cam.H && px.col < cam.W;
    const uint32_t r = px.row < cam.H ? px.row : cam.H - 1u, c = px.col < cam.W ? px.col : cam.W - 1u;
    Rng rng{sample_key(pd.seed, cam, r, c, 0u), 0};
    V3 o, d;
    sample_ray(cam, r, c, rng, o, d);
    double t = 0.0;
    uint32_t prim = 0xffffffffu;
    const bool hit = lane_query<COMPACT>(sc, o, d, stack, t, prim);
    V3 p = mk(0.0, 0.0, 0.0), n = mk(0.0, 0.0, 0.0);
    if (hit) {
        const PrimRec<COMPACT> rec = load_prim<COMPACT>(sc.prims, prim);
        p = hit_position(o, d, t);
        n = hit_point<COMPACT>(rec, p, d).normal;
        if (v_dot(n, d) > 0.0) n = v_scale(n, -1.0);
    }
    if (!inside) return;
    const size_t pix = (size_t)px.row * cam.W + px.col;
    pd.position[3 * pix] = p.x, pd.position[3 * pix + 1] = p.y, pd.position[3 * pix + 2] = p.z;
    pd.normal[3 * pix] = n.x, pd.normal[3 * pix + 1] = n.y, pd.normal[3 * pix + 2] = n.z;
    pd.active[pix] = hit ? (uint8_t)1 : (uint8_t)0;
}

hipError_t launch_ao(bool compact, const SceneDev& sc, const AoDev& ao, hipStream_t stream) {
    if (ao.n == 0u) return hipSuccess;
    const uint32_t lds = lane_stacks_lds_bytes(sc.stack_lds);
    const uint32_t blocks = (uint32_t)(ao_threads(ao.n, ao.block_points) / 256u);
    return with_bools([&](auto C, auto E, auto S) {
        auto kernel = &ao_kernel<decltype(C)::value, decltype(E)::value, decltype(S)::value>;
        const hipError_t e = raise_dynamic_lds(kernel, lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), lds, stream, sc, ao);
        return hipGetLastError();
    }, compact, sc.exact != 0u, ao.turns != nullptr);
}

hipError_t launch_ao_primary(bool compact, const SceneDev& sc, const CameraDev& cam, const AoPrimaryDev& pd, hipStream_t stream) {
    if (pd.n_tiles == 0u) return hipSuccess;
    const uint32_t lds = lane_stacks_lds_bytes(sc.stack_lds);
    const uint32_t blocks = (pd.n_tiles + 3u) / 4u;
    return with_bools([&](auto C) {
        auto kernel = &ao_primary_kernel<decltype(C)::value>;
        const hipError_t e = raise_dynamic_lds(kernel, lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), lds, stream, sc, cam, pd);
        return hipGetLastError();
    }, compact);
}

}  // namespace rayrs
