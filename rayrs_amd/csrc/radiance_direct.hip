// radiance_direct.hip -- the radiance queries with direct lighting (include/rayrs_hip.h DIRECT LIGHTING).  A unit of its own
// beside radiance_lit.hip: the kernels of the queries' three starts, the resolve and the launch.  The wave itself -- a lane walks
// TWO rays per diffuse bounce, the shadow ray and then the continuation -- is radiance_direct_wave.h's, which the direct-lit
// film's kernels (film_direct.hip) run with a start of their own.
#include <hip/hip_runtime.h>

#include "device_path.h"
#include "launch_dispatch.h"
#include "radiance_direct_kernels.h"
#include "radiance_direct_wave.h"
#include "radiance_wave_parts.h"

namespace rayrs {

// radiance_direct_wave.h's wave without the sky, its paths started by the queries: a batch's rays, points or pixels.
template <bool COMPACT, bool EXACT, int START>
__global__ void __launch_bounds__(256) radiance_direct_kernel(SceneDev sc, RadianceDev rd, LightsDev lights, LightSlotsDev slots, CameraDev cam) {
    extern __shared__ uint32_t lds_stack[];
    direct_wave<COMPACT, EXACT>(QueryStart<START>{}, lane_stack(lds_stack, rd.spill, sc), sc, rd, lights, slots, NoSky{}, cam);
}

__global__ void __launch_bounds__(256) radiance_direct_resolve_kernel(RadianceDev rd) { radiance_resolve(rd); }

hipError_t launch_radiance_direct(bool compact, const SceneDev& sc, const RadianceDev& rd, const LightsDev& lights,
                                  const LightSlotsDev& slots, const CameraDev& cam, int start, int cu_count, hipStream_t stream) {
    if (rd.n == 0u) return hipSuccess;
    const hipError_t e = with_lit_start([&](auto S) {
        return with_bools([&](auto C, auto E) {
            return launch_lane_stacks(&radiance_direct_kernel<decltype(C)::value, decltype(E)::value, decltype(S)::value>,
                                      radiance_grid_blocks(rd, cu_count), sc.stack_lds, stream, sc, rd, lights, slots, cam);
        }, compact, sc.exact != 0u);
    }, start);
    if (e != hipSuccess) return e;
    return launch_radiance_resolve(radiance_direct_resolve_kernel, rd, stream);
}

}  // namespace rayrs
