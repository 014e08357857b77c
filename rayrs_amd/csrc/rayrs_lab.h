/*
 * rayrs_lab.h -- PRIVATE scheduling knobs of librayrs_hip.so, for tests/ and scripts/ubench/ only.
 *
 * Not part of the boundary a rayrs-lib maintainer binds (include/rayrs_hip.h): nothing here has a
 * reference counterpart, none of it changes a frame, and any of it may go away.  The public
 * header keeps the two settings a caller may legitimately choose (rayrs_tuning: pool size, route).
 * 0 = the built-in default everywhere.
 */
#ifndef RAYRS_LAB_H
#define RAYRS_LAB_H

#include <stdint.h>

#include "../../include/rayrs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    uint32_t refill_min;    /* traversal: refill a wave's idle lanes when fewer than this are traversing (52) */
    uint32_t leaf_min;      /* traversal: run a leaf phase once this many lanes stand on a leaf (the fast walk: 24) / have a leaf
                               group waiting (the default walk: 48) */
    uint32_t static_pct;    /* traversal: share of the pool's windows dealt round robin, 1..100 (50) */
    uint32_t stack_lds;     /* traversal: stack entries per lane kept in LDS, the rest in HBM (12; the default walk, whose
                               stack holds interior records only: 8) */
    uint32_t hot_records;   /* traversal: leading wide records copied to LDS, at most 256 (14 KiB worth; the default walk 10 KiB);
                               0xffffffff = none */
    uint32_t trav_blocks_per_cu; /* traversal workgroups per CU, at most what the occupancy query allows */
    uint32_t eager_light;   /* 1 = the hit and miss kernels request a path's entry of the light side array together
                               with its slot also where no surface emits (they do anyway where one does) */
    uint32_t local_reserve; /* local-pool route: items a wave takes from the counter at a time, 8..4096 */
    uint32_t local_segment_items; /* local-pool route: items per launch segment, >= 65536 (default 2^27); raised
                               as far as needed to keep a frame within 64 segments */
    uint32_t force_rccl;    /* rayrs_render_multi: run the RCCL reduce even when every handle sits on one device
                               (a one-device communicator: the call path of a multi-GPU node on a one-GPU box) */
    uint32_t gate_tree;     /* 1 = the fast walk (with closest-hit culling) over the gate tree instead of the tree
                               of single primitives: what rounds 2 and 3 walked, kept for the same-box A/B of
                               profiles/r04_tight_leaves.txt */
    uint32_t hot_group;     /* 0xffffffff = the default walk reads the whole gate tree also where the scene has a hot group
                               (layout.h HotGroupDev), and the kernels that make rays pre-test nothing: the walk of round 5,
                               kept for the same-box A/B */
    uint32_t leaf_wait;     /* traversal, default walk: run a leaf phase once this many lanes can do nothing but wait for one
                               (leaf groups queued, no record to visit) (16) */
    uint32_t flat_blocks_per_cu; /* gen / hit / miss kernels: workgroups per CU of their common grid, 1..64 (default: 8 .. 24 by the
                               pool's size, about nine windows a wave) */
} rayrs_lab_tuning;

/* Applies to the renders launched on this scene afterwards.  Waits for a render in flight. */
int rayrs_lab_set(rayrs_scene* scene, const rayrs_lab_tuning* lab);

/* The entries of a lane's traversal stack on the scene's tree `which` (0: the fast walk's, 1: the gate tree, 2: the gate tree
 * without the hot group), what the overflow strips are sized by: rayrs_scene_info_t's depth of that tree, or what the walk of a
 * ray that enters every slot of every record -- an all-NaN ray -- needs if that is more (scene_host.cpp emit_wide).  Needs no
 * device.  Negative: rayrs_status (no scene, no such tree). */
int rayrs_lab_stack_need(rayrs_scene* scene, uint32_t which);

/* HIP-event times (ms) of the last finished render's path rounds, three per round: traversal, hit, miss kernel (the
 * local-pool route: its launch, 0, 0).  Returns the number of rounds (negative: rayrs_status); writes min(rounds,
 * cap_rounds) * 3 floats. */
int rayrs_lab_round_ms(rayrs_scene* scene, float* out, uint32_t cap_rounds);

/* The calls rayrs_render_multi's reduce makes for ranks on these devices -- the plan (which rank leads a device, which
 * are summed on it first), ncclCommInitAll once per device list, the grouped in-place ncclReduce to root 0, the syncs --
 * `rounds` times against a RECORDING table instead of librccl and the HIP runtime: no GPU is touched, so the path a node
 * of N distinct devices takes can be checked on a box that has none (tests/test_multi_plan.py).  fail_reduce_at >= 0: that
 * ncclReduce (counted over all rounds) reports an error.  log: ';'-separated record.  Returns the first non-OK status. */
int rayrs_lab_multi_rehearse(const int* rank_devices, uint32_t n, uint32_t rounds, int fail_reduce_at, char* log, uint32_t cap);

/* rayrs_scene_occluded (include/rayrs_hip.h RAY QUERIES) on host buffers through an instance of its kernel that also counts:
 * steps[i] = the turns of the any-hit walk's loop ray i took (records visited + leaf groups tested) before it finished.  With
 * a NaN t_max no ray stops early: the count is then the closest-hit query's on the same tree.  For scripts/ubench/query_bench.py's
 * measure of how much of a wave idles (64 consecutive rays share a wave, which runs as long as its slowest lane).  Refusals as
 * rayrs_scene_occluded's; steps is required. */
int rayrs_lab_query_steps(rayrs_scene* scene, const double* origin, const double* direction, const double* t_max, uint64_t n,
                          uint32_t fast_traversal, uint8_t* occluded, uint32_t* steps);

/* Ambient occlusion (include/rayrs_hip.h AMBIENT OCCLUSION): a wave of ao.hip's kernel hands its idle lanes new (point, sample)
 * items when fewer than refill_below lanes are walking, 1..64; 64 = whenever a lane is idle, 1 = only when none walks (no refill
 * within a batch of 64).  0 restores the default.  The counts are the same for every setting.  Applies to the calls on this
 * scene afterwards; RAYRS_INVALID_ARG above 64. */
int rayrs_lab_ao_refill(rayrs_scene* scene, uint32_t refill_below);

/* rayrs_scene_ambient_occlusion on host buffers through an instance of its kernel that also counts (never a timed one): turns[0]
 * = 64 x the step turns the waves took, turns[1] = the lane-turns of them in which a lane advanced its walk -- their quotient is
 * the share of lane-turns spent walking (scripts/ubench/ao_bench.py).  Refusals as rayrs_scene_ambient_occlusion's; count and
 * turns are required. */
int rayrs_lab_ao_turns(rayrs_scene* scene, const double* position, const double* normal, uint64_t n, uint32_t samples, double t_max,
                       double bias, uint64_t seed, uint64_t index_base, uint32_t fast_traversal, uint32_t* count, uint64_t turns[2]);

/* Radiance queries (include/rayrs_hip.h RADIANCE QUERY, IRRADIANCE): the thresholds of a wave of radiance.hip's kernel, 1..64
 * each.  refill_below: idle lanes take new (ray, chunk) items when fewer than this many lanes are walking (64 = whenever a lane is
 * idle, 1 = only when none walks).  shade_at: finished lanes are shaded once there are this many (1 = at once, 64 = only when no
 * lane walks; they always are when none walks).  leaf_min: a leaf phase runs once this many lanes stand on a leaf group.  0
 * restores a default (1, 64, 1: radiance_kernels.h, chosen by scripts/ubench/radiance_bench.py's sweep, profiles/radiance_rates.txt).
 * Every answer is the same bits under every setting: a chunk's sum is made in one lane in sample order, the rest by the resolve
 * in chunk order.  Applies to the calls on this scene afterwards; RAYRS_INVALID_ARG above 64. */
int rayrs_lab_radiance_tuning(rayrs_scene* scene, uint32_t refill_below, uint32_t shade_at, uint32_t leaf_min);

/* rayrs_scene_radiance (irradiance = 0: a = origins, b = directions; bias unused) or rayrs_scene_irradiance (irradiance = 1: a =
 * points, b = normals) on host buffers through an instance of the kernel that also counts (never a timed one): turns[0] = 64 x the
 * turns the waves took, turns[1] = the lane-turns in which a lane advanced its walk, turns[2] = those in which a lane was
 * shaded (scripts/ubench/radiance_bench.py).  Refusals as the entry points'; queries and turns are required. */
int rayrs_lab_radiance_turns(rayrs_scene* scene, uint32_t irradiance, const double* a, const double* b, uint64_t n, uint32_t samples,
                             uint32_t max_bounces, uint32_t sample_chunk, double bias, uint64_t seed, uint64_t index_base,
                             uint32_t fast_traversal, uint32_t* queries, uint64_t turns[3]);

/* SH PROBES' projection alone (radiance_probe.hip probe_project_kernel and probe_gather_kernel, in their rounds): `repeats` times
 * on the null stream over n probes of `samples` samples, n * samples <= 2^20, reading whatever the scene's radiance scratch
 * holds (the last probe call's paths; the projection's time does not depend on the values) and writing to the host forms'
 * staging, between two HIP events behind a warm-up; *ms is the mean of one (scripts/ubench/probes_bench.py).  Waits for the
 * scene's work first. */
int rayrs_lab_probe_project_ms(rayrs_scene* scene, uint32_t n, uint32_t samples, uint32_t sample_chunk, uint32_t repeats, float* ms);

/* LIGHTMAP ATLAS: the HIP-event times of the atlas's rayrs_lightmap_create, in milliseconds -- the owner pass (the plane's fill
 * included), the compaction's count and scan, the record pass (the list's allocation included)
 * (scripts/ubench/lightmap_bench.py). */
int rayrs_lab_lightmap_ms(const rayrs_lightmap* lightmap, double ms[3]);

#ifdef __cplusplus
}
#endif
#endif
