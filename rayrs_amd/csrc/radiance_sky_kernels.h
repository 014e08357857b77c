// radiance_sky_kernels.h -- the radiance queries with the sky among the lights (include/rayrs_hip.h SKY SAMPLING:
// rayrs_scene_radiance_sky, rayrs_scene_irradiance_sky, their _launch forms and rayrs_render_sky): what radiance_sky.hip's kernels
// are handed beside the direct kernels' arguments, and their launch wrapper.  The items, the scratch, the chunk rule, the
// thresholds, the light table, the slots and the three starts are radiance_kernels.h's, radiance_lit_kernels.h's and
// radiance_direct_kernels.h's; the sky's table is radiance_sky_table.h's SkyDev.
#pragma once
#include <hip/hip_runtime.h>

#include "radiance_direct_kernels.h"
#include "radiance_sky_table.h"

namespace rayrs {

// radiance_sky_kernel on a grid of at most cu_count * RADIANCE_BLOCKS_PER_CU workgroups, then radiance_sky_resolve_kernel.
// start: LIT_START_*; cam is read by LIT_START_PIXEL only, rd.a and rd.b by the other two.  lights.n may be 0: the sky alone.
hipError_t launch_radiance_sky(bool compact, const SceneDev& sc, const RadianceDev& rd, const LightsDev& lights, const LightSlotsDev& slots,
                               const SkyDev& sky, const CameraDev& cam, int start, int cu_count, hipStream_t stream);

}  // namespace rayrs
