// radiance_lit_kernels.h -- the radiance queries with light sampling (include/rayrs_hip.h LIGHT SAMPLING: rayrs_scene_radiance_lit,
// rayrs_scene_irradiance_lit, their _launch forms and rayrs_render_lit): what radiance_lit.hip's kernels are handed, and their
// launch wrapper.  The items, the scratch, the chunk rule and the thresholds are radiance_kernels.h's.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/rayrs_hip.h"
#include "layout.h"
#include "radiance_kernels.h"

namespace rayrs {

// One light of the list, resolved on the host (radiance_lit_abi.cpp lights_resolve) from the object's primitive record: what
// Hittable::sample and the density read, nothing the kernel has to fetch.
//   sphere (PRIM_SPHERE): radius2, centre x y z, radius = sqrt(radius2), area = (4.0 * RR_PI) * radius2, 0
//   plane  (PRIM_PLANE):  umin, umax, vmin, vmax, pos, area = (umax - umin) * (vmax - vmin), 0
struct LightDev {
    uint32_t kind;  // PRIM_SPHERE or PRIM_PLANE
    uint32_t axis;  // the plane's Axis (geometry.rs:161-168)
    double v[7];
};
static_assert(sizeof(LightDev) == 64, "LightDev");

// The list, passed BY VALUE in the kernel arguments: a _launch call orders no copy for it.
struct LightsDev {
    uint32_t n;  // K, 0 .. RAYRS_MAX_LIGHTS; 0: Material::evaluate(.., None)
    uint32_t pad;
    LightDev light[RAYRS_MAX_LIGHTS];
};

// How a sample starts: the caller's ray, draw 0 next; the irradiance point, whose first direction is the operation's at (p + n *
// bias, n) with albedo (1, 1, 1) -- with K = 0 IRRADIANCE's ray on draws 0 and 1 --; the camera's pixel, sample_ray on draws
// 0 and 1, draw 2 next.
constexpr int LIT_START_RAY = 0, LIT_START_POINT = 1, LIT_START_PIXEL = 2;
// SH PROBES' start (radiance_probe_kernels.h ProbeStart, never a with_lit_start value): the ray leaves the probe's point along
// the direction made on draws 0 and 1, draw 2 next; there is no second array and no virtual bounce.
constexpr int LIT_START_PROBE = 3;
// with_lit_start(f, start) calls f(S) with S() the LIT_START_* that `start` is, as launch_dispatch.h's with_bools does for bools.
template <class F>
auto with_lit_start(F f, int start) {
    if (start == LIT_START_PIXEL) return f(std::integral_constant<int, LIT_START_PIXEL>{});
    if (start == LIT_START_POINT) return f(std::integral_constant<int, LIT_START_POINT>{});
    return f(std::integral_constant<int, LIT_START_RAY>{});
}

// radiance_lit_kernel on a grid of at most cu_count * RADIANCE_BLOCKS_PER_CU workgroups, then radiance_lit_resolve_kernel.
// start: LIT_START_*; cam is read by LIT_START_PIXEL only, rd.a and rd.b by the other two.
hipError_t launch_radiance_lit(bool compact, const SceneDev& sc, const RadianceDev& rd, const LightsDev& lights, const CameraDev& cam,
                               int start, int cu_count, hipStream_t stream);

}  // namespace rayrs
