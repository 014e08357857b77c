// radiance_direct_kernels.h -- the radiance queries with direct lighting (include/rayrs_hip.h DIRECT LIGHTING:
// rayrs_scene_radiance_direct, rayrs_scene_irradiance_direct, their _launch forms and rayrs_render_direct): what
// radiance_direct.hip's kernels are handed beside the lit kernels' arguments, and their launch wrapper.  The items, the scratch, the
// chunk rule, the thresholds, the light table and the three starts are radiance_kernels.h's and radiance_lit_kernels.h's.
#pragma once
#include <hip/hip_runtime.h>

#include "radiance_lit_kernels.h"

namespace rayrs {

// The list once more, as the depth-first slots a walk answers with (Trav::best_prim): "is the hit object in the list" is a
// comparison against these, slot k for light k of LightsDev.  BY VALUE in the kernel arguments, as the table is.
struct LightSlotsDev {
    uint32_t prim[RAYRS_MAX_LIGHTS];
};

// radiance_direct_kernel on a grid of at most cu_count * RADIANCE_BLOCKS_PER_CU workgroups, then radiance_direct_resolve_kernel.
// start: LIT_START_*; cam is read by LIT_START_PIXEL only, rd.a and rd.b by the other two.
hipError_t launch_radiance_direct(bool compact, const SceneDev& sc, const RadianceDev& rd, const LightsDev& lights,
                                  const LightSlotsDev& slots, const CameraDev& cam, int start, int cu_count, hipStream_t stream);

}  // namespace rayrs
