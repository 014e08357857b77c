// radiance_mesh_kernels.h -- the radiance queries with a mesh-light group among the lights (include/rayrs_hip.h MESH LIGHTS:
// rayrs_scene_radiance_mesh, rayrs_scene_irradiance_mesh, their _launch forms and rayrs_render_mesh): what radiance_mesh.hip's
// kernels are handed beside the sky kernels' arguments, and their launch wrapper.  The items, the scratch, the chunk rule, the
// thresholds, the light table, the slots, the sky's table and the three starts are radiance_kernels.h's, radiance_lit_kernels.h's,
// radiance_direct_kernels.h's and radiance_sky_kernels.h's; the group is radiance_mesh_table.h's MeshDev.
#pragma once
#include <hip/hip_runtime.h>

#include "radiance_mesh_table.h"
#include "radiance_sky_kernels.h"

namespace rayrs {

// radiance_mesh_kernel on a grid of at most cu_count * RADIANCE_BLOCKS_PER_CU workgroups, then radiance_mesh_resolve_kernel.
// mesh.n >= 1 (a call with an empty group is DIRECT LIGHTING's or SKY SAMPLING's).  with_sky: the sky is the last light, and
// `sky` its table; otherwise `sky` is not read.  start: LIT_START_*; cam is read by LIT_START_PIXEL only, rd.a and rd.b by the
// other two.  lights.n may be 0: the group alone, or with the sky.
hipError_t launch_radiance_mesh(bool compact, const SceneDev& sc, const RadianceDev& rd, const LightsDev& lights, const LightSlotsDev& slots,
                                const MeshDev& mesh, const SkyDev& sky, bool with_sky, const CameraDev& cam, int start, int cu_count,
                                hipStream_t stream);

}  // namespace rayrs
