// radiance_probe.hip -- SH probes (include/rayrs_hip.h SH PROBES).  A unit of its own: the direct wave without and with the sky
// (radiance_direct_wave.h) and the group wave with the area and the tree's group (radiance_group_wave.h), started by the probes
// (radiance_probe_kernels.h ProbeStart: an item is one sample of one probe), and the projection behind them, which takes
// radiance_resolve's place: every sample's direction made again from its key, the nine harmonics, and the sums in the header's
// order.  The waves keep no accumulator of the projection: they stand at 200 to 230 VGPRs as they are.
#include <hip/hip_runtime.h>

#include "device_path.h"
#include "launch_dispatch.h"
#include "radiance_direct_wave.h"
#include "radiance_group_wave.h"
#include "radiance_probe_kernels.h"
#include "radiance_wave_parts.h"

namespace rayrs {

template <bool COMPACT, bool EXACT>
__global__ void __launch_bounds__(256) probe_direct_kernel(SceneDev sc, RadianceDev rd, LightsDev lights, LightSlotsDev slots, CameraDev cam) {
    extern __shared__ uint32_t lds_stack[];
    direct_wave<COMPACT, EXACT>(ProbeStart{}, lane_stack(lds_stack, rd.spill, sc), sc, rd, lights, slots, NoSky{}, cam);
}

template <bool COMPACT, bool EXACT>
__global__ void __launch_bounds__(256) probe_sky_kernel(SceneDev sc, RadianceDev rd, LightsDev lights, LightSlotsDev slots, SkyDev sky, CameraDev cam) {
    extern __shared__ uint32_t lds_stack[];
    direct_wave<COMPACT, EXACT>(ProbeStart{}, lane_stack(lds_stack, rd.spill, sc), sc, rd, lights, slots, sky, cam);
}

template <bool COMPACT, bool EXACT, bool SKY>
__global__ void __launch_bounds__(256) probe_mesh_kernel(SceneDev sc, RadianceDev rd, LightsDev lights, LightSlotsDev slots, MeshDev mesh, SkyDev sky, CameraDev cam) {
    extern __shared__ uint32_t lds_stack[];
    group_wave<COMPACT, EXACT, SKY>(ProbeStart{}, lane_stack(lds_stack, rd.spill, sc), sc, rd, lights, slots, mesh, sky, cam);
}

template <bool COMPACT, bool EXACT, bool SKY>
__global__ void __launch_bounds__(256) probe_tree_kernel(SceneDev sc, RadianceDev rd, LightsDev lights, LightSlotsDev slots, TreeDev tree, SkyDev sky, CameraDev cam) {
    extern __shared__ uint32_t lds_stack[];
    group_wave<COMPACT, EXACT, SKY>(ProbeStart{}, lane_stack(lds_stack, rd.spill, sc), sc, rd, lights, slots, tree, sky, cam);
}

// One thread per (probe, chunk) pair of the round: C[k][ch] from zero, for each sample of the chunk in sample order
// += Y_k * L_s[ch] (one multiplication, then one addition), and the chunk's query count.  27 sums in registers; every index
// below is a constant once the loops over k and ch are unrolled.
__global__ void __launch_bounds__(256) probe_project_kernel(ProbeDev pd) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= pd.pairs) return;
    const uint32_t pair = pd.pair0 + t;
    const uint32_t probe = pair / pd.chunks;
    const uint32_t s0 = (pair - probe * pd.chunks) * pd.chunk;
    const uint32_t s1 = pd.samples - s0 < pd.chunk ? pd.samples : s0 + pd.chunk;
    const double* L = pd.partial + ((size_t)probe * pd.samples + s0) * 3u;
    const uint32_t* Lq = pd.partial_queries + ((size_t)probe * pd.samples + s0);
    double C[PROBE_PLANES];
#pragma unroll
    for (uint32_t c = 0; c < PROBE_PLANES; c++) C[c] = 0.0;
    uint32_t q = 0u;
    for (uint32_t s = s0; s < s1; s++, L += 3, Lq++) {
        double w[3], Y[SH_COEFFS];
        probe_sample_direction(pd.seed, pd.index_base + probe, s, w);
        sh_basis(w[0], w[1], w[2], Y);
        const double l[3] = {L[0], L[1], L[2]};
#pragma unroll
        for (uint32_t k = 0; k < SH_COEFFS; k++) {
#pragma unroll
            for (uint32_t ch = 0; ch < 3u; ch++) {
                const double term = Y[k] * l[ch];
                C[k * 3u + ch] = C[k * 3u + ch] + term;
            }
        }
        q += *Lq;
    }
#pragma unroll
    for (uint32_t c = 0; c < PROBE_PLANES; c++) pd.slots[(size_t)c * PROBE_CHUNK_SLOTS + t] = C[c];
    pd.slot_queries[t] = q;
}

// One thread per (probe of the round, c): c < 27 is the plane k * 3 + ch, c == 27 the query count.  The probe's chunks that lie
// in the round are added in chunk order: the probe's first chunk is assigned, a later round goes on from what the last one left
// in coeffs (queries), and the round that holds the probe's last chunk scales the sum.
__global__ void __launch_bounds__(256) probe_gather_kernel(ProbeDev pd) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const uint32_t first_probe = pd.pair0 / pd.chunks;
    const uint32_t probe = first_probe + t / (PROBE_PLANES + 1u);
    const uint32_t c = t - (t / (PROBE_PLANES + 1u)) * (PROBE_PLANES + 1u);
    const uint32_t end = pd.pair0 + pd.pairs;
    if (probe >= pd.n || (unsigned long long)probe * pd.chunks >= end) return;
    const uint32_t p_first = probe * pd.chunks;  // (below end <= n * chunks <= 2^20)
    const uint32_t p_end = p_first + pd.chunks;
    const uint32_t lo = p_first > pd.pair0 ? p_first : pd.pair0;
    const uint32_t hi = p_end < end ? p_end : end;
    if (c == PROBE_PLANES) {
        if (pd.queries == nullptr) return;
        uint32_t q = lo == p_first ? 0u : pd.queries[probe];
        for (uint32_t p = lo; p < hi; p++) q += pd.slot_queries[p - pd.pair0];
        pd.queries[probe] = q;
        return;
    }
    const double* plane = pd.slots + (size_t)c * PROBE_CHUNK_SLOTS;
    double* dst = pd.coeffs + (size_t)probe * PROBE_PLANES + c;
    double sum;
    uint32_t p = lo;
    if (lo == p_first) sum = plane[p - pd.pair0], p++;  // C_0 assigned
    else sum = *dst;
    for (; p < hi; p++) sum = sum + plane[p - pd.pair0];
    if (hi == p_end) {
        const double four_pi = 4.0 * RR_PI;
        sum = sum * (four_pi * (1.0 / (double)pd.samples));
    }
    *dst = sum;
}

hipError_t launch_probe_wave(bool compact, const SceneDev& sc, const RadianceDev& rd, const LightsDev& lights, const LightSlotsDev& slots,
                             const MeshDev* mesh, const TreeDev* tree, const SkyDev& sky, bool with_sky, int cu_count, hipStream_t stream) {
    if (rd.n == 0u) return hipSuccess;
    const CameraDev cam{};  // (read by LIT_START_PIXEL only)
    const uint32_t blocks = radiance_grid_blocks(rd, cu_count);
    if (tree != nullptr)
        return with_bools([&](auto C, auto E, auto K) {
            return launch_lane_stacks(&probe_tree_kernel<decltype(C)::value, decltype(E)::value, decltype(K)::value>, blocks, sc.stack_lds,
                                      stream, sc, rd, lights, slots, *tree, sky, cam);
        }, compact, sc.exact != 0u, with_sky);
    if (mesh != nullptr)
        return with_bools([&](auto C, auto E, auto K) {
            return launch_lane_stacks(&probe_mesh_kernel<decltype(C)::value, decltype(E)::value, decltype(K)::value>, blocks, sc.stack_lds,
                                      stream, sc, rd, lights, slots, *mesh, sky, cam);
        }, compact, sc.exact != 0u, with_sky);
    return with_bools([&](auto C, auto E) {
        if (with_sky)
            return launch_lane_stacks(&probe_sky_kernel<decltype(C)::value, decltype(E)::value>, blocks, sc.stack_lds, stream, sc, rd,
                                      lights, slots, sky, cam);
        return launch_lane_stacks(&probe_direct_kernel<decltype(C)::value, decltype(E)::value>, blocks, sc.stack_lds, stream, sc, rd,
                                  lights, slots, cam);
    }, compact, sc.exact != 0u);
}

hipError_t launch_probe_project(const ProbeDev& pd, hipStream_t stream) {
    if (pd.pairs == 0u) return hipSuccess;
    hipLaunchKernelGGL(probe_project_kernel, dim3((pd.pairs + 255u) / 256u), dim3(256), 0, stream, pd);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const uint32_t first_probe = pd.pair0 / pd.chunks;
    const uint32_t last_probe = (pd.pair0 + pd.pairs - 1u) / pd.chunks;
    const uint32_t threads = (last_probe - first_probe + 1u) * (PROBE_PLANES + 1u);
    hipLaunchKernelGGL(probe_gather_kernel, dim3((threads + 255u) / 256u), dim3(256), 0, stream, pd);
    return hipGetLastError();
}

}  // namespace rayrs
