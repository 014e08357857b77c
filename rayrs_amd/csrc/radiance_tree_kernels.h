// radiance_tree_kernels.h -- the radiance queries with a mesh-light group chosen by a light tree (include/rayrs_hip.h LIGHT TREE;
// the entry points are MESH LIGHTS', handed a rayrs_mesh_lights_create_tree handle): what radiance_tree.hip's kernels are handed
// beside the sky kernels' arguments, and their launch wrapper.  Everything but the group is radiance_mesh_kernels.h's; the group
// is radiance_tree_table.h's TreeDev.
#pragma once
#include <hip/hip_runtime.h>

#include "radiance_sky_kernels.h"
#include "radiance_tree_table.h"

namespace rayrs {

// radiance_tree_kernel on a grid of at most cu_count * RADIANCE_BLOCKS_PER_CU workgroups, then radiance_tree_resolve_kernel.
// tree.n >= 1 (a call with an empty group is DIRECT LIGHTING's or SKY SAMPLING's).  The other arguments are
// launch_radiance_mesh's.
hipError_t launch_radiance_tree(bool compact, const SceneDev& sc, const RadianceDev& rd, const LightsDev& lights, const LightSlotsDev& slots,
                                const TreeDev& tree, const SkyDev& sky, bool with_sky, const CameraDev& cam, int start, int cu_count,
                                hipStream_t stream);

}  // namespace rayrs
