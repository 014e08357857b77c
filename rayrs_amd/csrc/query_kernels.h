// query_kernels.h -- ray queries on caller rays (include/rayrs_hip.h RAY QUERIES: rayrs_scene_intersect,
// rayrs_scene_occluded and their _launch forms): what query.hip's kernels are handed, and their launch wrappers.
#pragma once
#include <hip/hip_runtime.h>

#include "layout.h"

namespace rayrs {

// One launch of a query: the rays 0 .. n - 1 behind these pointers (query_abi.cpp moves them on from launch to launch),
// one ray per thread.  A launch holds at most QUERY_LAUNCH_RAYS rays, which bounds the stack strip.
constexpr uint64_t QUERY_LAUNCH_RAYS = 1ull << 20;
struct QueryDev {
    uint32_t n;
    uint32_t n_prims;             // entries of prim_object
    const double* origin;         // n * 3
    const double* direction;      // n * 3
    const double* t_max;          // n, or null = +infinity for every ray (the occlusion query)
    const uint32_t* prim_object;  // depth-first slot -> object in insertion order (the closest-hit query)
    double* t;                    // n
    uint32_t* object;             // n
    double* normal;               // n * 3, or null = not wanted
    uint8_t* occluded;            // n
    uint32_t* steps;              // n, or null: the turns of the any-hit walk's loop each ray took (rayrs_lab_query_steps only)
    uint32_t* spill;              // the traversal stacks' overflow: (stack_depth - stack_lds) words per thread of the grid
};

// threads of a query's grid (whole 256-thread workgroups): sizes the spill strip
inline uint64_t query_threads(uint64_t n) { return (n + 255u) / 256u * 256u; }
hipError_t launch_query_intersect(bool compact, const SceneDev& sc, const QueryDev& q, hipStream_t stream);
hipError_t launch_query_occluded(bool compact, const SceneDev& sc, const QueryDev& q, hipStream_t stream);

}  // namespace rayrs
