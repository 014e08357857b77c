// bake_mesh.hip -- the mesh-lit bakes (include/rayrs_hip.h MESH-LIT FILMS AND BAKES): the bake's wave kernels with a mesh-light
// group among the lights.  They are radiance_group_wave.h's wave, started per (entry, chunk) item of a pass's sample window
// (bake_kernels.h BakeStart); bake.hip's bake_accumulate_kernel follows every launch on the same stream, unchanged, and the
// select, the status, the noise and the read are bake.hip's.  A unit of its own, as radiance_mesh.hip is beside
// radiance_direct.hip.  No arithmetic of a sample is written here: a chunk's sum is the wave's.
#include <hip/hip_runtime.h>

#include "device_path.h"
#include "launch_dispatch.h"
#include "passes_mesh_kernels.h"
#include "radiance_group_wave.h"

namespace rayrs {

template <bool COMPACT, bool EXACT, bool SKY, int KIND>
__global__ void __launch_bounds__(256) bake_mesh_kernel(SceneDev sc, RadianceDev rd, BakeStartDev bs, LightsDev lights, LightSlotsDev slots,
                                                        MeshDev mesh, SkyDev sky) {
    extern __shared__ uint32_t lds_stack[];
    const CameraDev cam{};  // (read by LIT_START_PIXEL only: never here)
    group_wave<COMPACT, EXACT, SKY>(BakeStart<KIND>{bs}, lane_stack(lds_stack, rd.spill, sc), sc, rd, lights, slots, mesh, sky, cam);
}

hipError_t launch_bake_mesh(bool compact, const SceneDev& sc, const RadianceDev& rd, const BakeStartDev& bs, const LightsDev& lights,
                            const LightSlotsDev& slots, const MeshDev& mesh, const SkyDev& sky, bool with_sky, bool irradiance,
                            int cu_count, hipStream_t stream) {
    if (rd.n == 0u) return hipSuccess;
    const uint32_t blocks = radiance_grid_blocks(rd, cu_count);
    return with_bools([&](auto C, auto E, auto K, auto P) {
        constexpr int KIND = decltype(P)::value ? LIT_START_POINT : LIT_START_RAY;
        return launch_lane_stacks(&bake_mesh_kernel<decltype(C)::value, decltype(E)::value, decltype(K)::value, KIND>, blocks, sc.stack_lds,
                                  stream, sc, rd, bs, lights, slots, mesh, sky);
    }, compact, sc.exact != 0u, with_sky, irradiance);
}

}  // namespace rayrs
