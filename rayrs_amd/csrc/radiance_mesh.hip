// radiance_mesh.hip -- the radiance queries with a mesh-light group among the lights of direct lighting (include/rayrs_hip.h MESH
// LIGHTS).  A unit of its own beside radiance_direct.hip and radiance_sky.hip: the kernels of the queries' three starts, without
// and with the sky, the resolve and the launch.  The wave itself, and what sets it apart from the direct wave, is
// radiance_group_wave.h's, which radiance_tree.hip's kernels run with the tree's group.
#include <hip/hip_runtime.h>

#include "device_path.h"
#include "launch_dispatch.h"
#include "radiance_mesh_kernels.h"
#include "radiance_group_wave.h"
#include "radiance_wave_parts.h"

namespace rayrs {

// radiance_group_wave.h's wave with the area group, its paths started by the queries: a batch's rays, points or pixels.
template <bool COMPACT, bool EXACT, bool SKY, int START>
__global__ void __launch_bounds__(256) radiance_mesh_kernel(SceneDev sc, RadianceDev rd, LightsDev lights, LightSlotsDev slots, MeshDev mesh, SkyDev sky, CameraDev cam) {
    extern __shared__ uint32_t lds_stack[];
    group_wave<COMPACT, EXACT, SKY>(QueryStart<START>{}, lane_stack(lds_stack, rd.spill, sc), sc, rd, lights, slots, mesh, sky, cam);
}

__global__ void __launch_bounds__(256) radiance_mesh_resolve_kernel(RadianceDev rd) { radiance_resolve(rd); }

hipError_t launch_radiance_mesh(bool compact, const SceneDev& sc, const RadianceDev& rd, const LightsDev& lights, const LightSlotsDev& slots,
                                const MeshDev& mesh, const SkyDev& sky, bool with_sky, const CameraDev& cam, int start, int cu_count,
                                hipStream_t stream) {
    if (rd.n == 0u) return hipSuccess;
    const hipError_t e = with_lit_start([&](auto S) {
        return with_bools([&](auto C, auto E, auto K) {
            return launch_lane_stacks(&radiance_mesh_kernel<decltype(C)::value, decltype(E)::value, decltype(K)::value, decltype(S)::value>,
                                      radiance_grid_blocks(rd, cu_count), sc.stack_lds, stream, sc, rd, lights, slots, mesh, sky, cam);
        }, compact, sc.exact != 0u, with_sky);
    }, start);
    if (e != hipSuccess) return e;
    return launch_radiance_resolve(radiance_mesh_resolve_kernel, rd, stream);
}

}  // namespace rayrs
