// passes_mesh_kernels.h -- the mesh-lit films and bakes (include/rayrs_hip.h MESH-LIT FILMS AND BAKES: rayrs_film_create_mesh,
// rayrs_bake_create_mesh): the launch wrappers of film_mesh.hip's and bake_mesh.hip's kernels, which are radiance_group_wave.h's
// wave started by a film pass (film_direct_kernels.h FilmStart) and by a bake pass (bake_kernels.h BakeStart).  Everything else
// of a pass -- the scratch, the item numbering, the counts, the accumulate kernels -- is the direct-lit film's and the bake's.
#pragma once
#include <hip/hip_runtime.h>

#include "bake_kernels.h"
#include "film_direct_kernels.h"
#include "radiance_mesh_table.h"

namespace rayrs {

// film_mesh_kernel on launch_film_direct's grid, its items, sums and counts where that launch leaves them.  mesh.n >= 1 (a film
// with an empty group launches film_direct.hip's kernels).  with_sky: the sky is the last light, and `sky` its table; otherwise
// `sky` is not read.  lights.n may be 0.
hipError_t launch_film_mesh(bool compact, const SceneDev& sc, const RadianceDev& rd, const FilmStartDev& fs, const LightsDev& lights,
                            const LightSlotsDev& slots, const MeshDev& mesh, const SkyDev& sky, bool with_sky, const CameraDev& cam,
                            int cu_count, hipStream_t stream);
// bake_mesh_kernel on launch_bake_wave's grid, the same way.  irradiance: LIT_START_POINT, else LIT_START_RAY.
hipError_t launch_bake_mesh(bool compact, const SceneDev& sc, const RadianceDev& rd, const BakeStartDev& bs, const LightsDev& lights,
                            const LightSlotsDev& slots, const MeshDev& mesh, const SkyDev& sky, bool with_sky, bool irradiance,
                            int cu_count, hipStream_t stream);

}  // namespace rayrs
