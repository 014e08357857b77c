// radiance_sky.hip -- the radiance queries with the sky among the lights of direct lighting (include/rayrs_hip.h SKY SAMPLING).
// A unit of its own beside radiance_direct.hip: the kernels of the queries' three starts, the resolve and the launch.  The wave
// itself is radiance_direct_wave.h's, handed the sky; what the sky changes in it is said there.
#include <hip/hip_runtime.h>

#include "device_path.h"
#include "launch_dispatch.h"
#include "radiance_direct_wave.h"
#include "radiance_sky_kernels.h"
#include "radiance_wave_parts.h"

namespace rayrs {

// radiance_direct_wave.h's wave with the sky, its paths started by the queries: a batch's rays, points or pixels.
template <bool COMPACT, bool EXACT, int START>
__global__ void __launch_bounds__(256) radiance_sky_kernel(SceneDev sc, RadianceDev rd, LightsDev lights, LightSlotsDev slots, SkyDev sky, CameraDev cam) {
    extern __shared__ uint32_t lds_stack[];
    direct_wave<COMPACT, EXACT>(QueryStart<START>{}, lane_stack(lds_stack, rd.spill, sc), sc, rd, lights, slots, sky, cam);
}

__global__ void __launch_bounds__(256) radiance_sky_resolve_kernel(RadianceDev rd) { radiance_resolve(rd); }

hipError_t launch_radiance_sky(bool compact, const SceneDev& sc, const RadianceDev& rd, const LightsDev& lights, const LightSlotsDev& slots,
                               const SkyDev& sky, const CameraDev& cam, int start, int cu_count, hipStream_t stream) {
    if (rd.n == 0u) return hipSuccess;
    const hipError_t e = with_lit_start([&](auto S) {
        return with_bools([&](auto C, auto E) {
            return launch_lane_stacks(&radiance_sky_kernel<decltype(C)::value, decltype(E)::value, decltype(S)::value>,
                                      radiance_grid_blocks(rd, cu_count), sc.stack_lds, stream, sc, rd, lights, slots, sky, cam);
        }, compact, sc.exact != 0u);
    }, start);
    if (e != hipSuccess) return e;
    return launch_radiance_resolve(radiance_sky_resolve_kernel, rd, stream);
}

}  // namespace rayrs
