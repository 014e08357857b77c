// film_mesh.hip -- the mesh-lit films (include/rayrs_hip.h MESH-LIT FILMS AND BAKES): a third producer of a film pass's chunk sums
// beside the path kernels and film_direct.hip's.  Its kernels are radiance_group_wave.h's wave, started per (tile, pixel, chunk)
// item of a pass's sample window (film_direct_kernels.h FilmStart); film_direct.hip's count kernel and film.hip's
// film_accumulate_kernel follow every launch on the same stream, unchanged.  A unit of its own, as radiance_mesh.hip is beside
// radiance_direct.hip.  No arithmetic of a sample is written here: a chunk's sum is the wave's.
#include <hip/hip_runtime.h>

#include "device_path.h"
#include "launch_dispatch.h"
#include "passes_mesh_kernels.h"
#include "radiance_group_wave.h"

namespace rayrs {

template <bool COMPACT, bool EXACT, bool SKY>
__global__ void __launch_bounds__(256) film_mesh_kernel(SceneDev sc, RadianceDev rd, FilmStartDev fs, LightsDev lights, LightSlotsDev slots,
                                                        MeshDev mesh, SkyDev sky, CameraDev cam) {
    extern __shared__ uint32_t lds_stack[];
    group_wave<COMPACT, EXACT, SKY>(FilmStart{fs}, lane_stack(lds_stack, rd.spill, sc), sc, rd, lights, slots, mesh, sky, cam);
}

hipError_t launch_film_mesh(bool compact, const SceneDev& sc, const RadianceDev& rd, const FilmStartDev& fs, const LightsDev& lights,
                            const LightSlotsDev& slots, const MeshDev& mesh, const SkyDev& sky, bool with_sky, const CameraDev& cam,
                            int cu_count, hipStream_t stream) {
    if (rd.n == 0u) return hipSuccess;
    const uint32_t blocks = radiance_grid_blocks(rd, cu_count);
    return with_bools([&](auto C, auto E, auto K) {
        return launch_lane_stacks(&film_mesh_kernel<decltype(C)::value, decltype(E)::value, decltype(K)::value>, blocks, sc.stack_lds, stream,
                                  sc, rd, fs, lights, slots, mesh, sky, cam);
    }, compact, sc.exact != 0u, with_sky);
}

}  // namespace rayrs
