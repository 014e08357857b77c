// film_direct.hip -- the direct-lit films (include/rayrs_hip.h DIRECT-LIT FILMS): a second producer of a film pass's chunk sums
// beside the path kernels of rayrs_render.  Its kernels are radiance_direct_wave.h's wave without and with the sky, started per
// (tile, pixel, chunk) item of a pass's sample window (film_direct_kernels.h FilmStart) in the numbering film.hip's
// film_accumulate_kernel reads, which follows every launch on the same stream; and a small kernel that adds up the launch's query
// counts and in-image pixels.  No arithmetic of a sample is written here: a chunk's sum is the waves'.
#include <hip/hip_runtime.h>

#include "device_path.h"
#include "film_direct_kernels.h"
#include "launch_dispatch.h"
#include "radiance_direct_wave.h"

namespace rayrs {

template <bool COMPACT, bool EXACT>
__global__ void __launch_bounds__(256) film_direct_kernel(SceneDev sc, RadianceDev rd, FilmStartDev fs, LightsDev lights, LightSlotsDev slots,
                                                          CameraDev cam) {
    extern __shared__ uint32_t lds_stack[];
    direct_wave<COMPACT, EXACT>(FilmStart{fs}, lane_stack(lds_stack, rd.spill, sc), sc, rd, lights, slots, NoSky{}, cam);
}

template <bool COMPACT, bool EXACT>
__global__ void __launch_bounds__(256) film_sky_kernel(SceneDev sc, RadianceDev rd, FilmStartDev fs, LightsDev lights, LightSlotsDev slots,
                                                       SkyDev sky, CameraDev cam) {
    extern __shared__ uint32_t lds_stack[];
    direct_wave<COMPACT, EXACT>(FilmStart{fs}, lane_stack(lds_stack, rd.spill, sc), sc, rd, lights, slots, sky, cam);
}

// One lane per item of the launch.  An item the start skipped stored no count and is not read; a pixel is counted at its first
// chunk.  Integers: a wave's lanes are added with cross-lane moves, then one atomic add per counter and wave, in any order.
__global__ void __launch_bounds__(256) film_direct_count_kernel(RadianceDev rd, FilmStartDev fs, CameraDev cam, uint32_t count_queries,
                                                                FilmDirectCounts* counts) {
    const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t n_items = (uint64_t)rd.n * rd.chunks;
    uint32_t q = 0u;
    bool first_chunk = false;
    if (idx < n_items) {
        uint32_t row, col, k, n_before;
        if (film_item_pixel(fs, cam, rd.chunks, (uint32_t)idx, row, col, k, n_before)) {
            if (count_queries) q = rd.partial_queries[idx];
            first_chunk = k == 0u;
        }
    }
    unsigned long long sum = q;  // (64 counts below 2^32 each)
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_down((int)(uint32_t)sum, off, 64);
        const uint32_t hi = (uint32_t)__shfl_down((int)(uint32_t)(sum >> 32), off, 64);
        sum += ((unsigned long long)hi << 32) | lo;
    }
    const unsigned long long b_pix = __ballot(first_chunk);
    if ((threadIdx.x & 63u) == 0u) {
        if (sum) atomicAdd(&counts->queries, sum);
        if (b_pix) atomicAdd(&counts->pixels, (unsigned long long)__popcll(b_pix));
    }
}

hipError_t launch_film_direct(bool compact, const SceneDev& sc, const RadianceDev& rd, const FilmStartDev& fs, const LightsDev& lights,
                              const LightSlotsDev& slots, const SkyDev* sky, const CameraDev& cam, int cu_count, hipStream_t stream) {
    if (rd.n == 0u) return hipSuccess;
    const uint32_t blocks = radiance_grid_blocks(rd, cu_count);
    return with_bools([&](auto C, auto E) {
        if (sky) return launch_lane_stacks(&film_sky_kernel<decltype(C)::value, decltype(E)::value>, blocks, sc.stack_lds, stream, sc, rd, fs,
                                           lights, slots, *sky, cam);
        return launch_lane_stacks(&film_direct_kernel<decltype(C)::value, decltype(E)::value>, blocks, sc.stack_lds, stream, sc, rd, fs, lights,
                                  slots, cam);
    }, compact, sc.exact != 0u);
}

hipError_t launch_film_direct_count(const RadianceDev& rd, const FilmStartDev& fs, const CameraDev& cam, uint32_t count_queries,
                                    FilmDirectCounts* counts, hipStream_t stream) {
    const uint64_t n_items = (uint64_t)rd.n * rd.chunks;
    if (n_items == 0u) return hipSuccess;
    hipLaunchKernelGGL(film_direct_count_kernel, dim3((uint32_t)((n_items + 255u) / 256u)), dim3(256), 0, stream, rd, fs, cam, count_queries,
                       counts);
    return hipGetLastError();
}

}  // namespace rayrs
