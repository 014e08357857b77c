// lightmap_kernels.h -- the lightmap atlas (include/rayrs_hip.h LIGHTMAP ATLAS: rayrs_lightmap_*): what lightmap.hip's kernels are
// handed, the triangle set-up and the edge functions written once for all of them, and the launch wrappers.  All f64, unfused, in
// the header's operation order.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace rayrs {

constexpr uint32_t LIGHTMAP_NO_OWNER = 0xFFFFFFFFu;
// The owner pass's three ways to walk a triangle's candidates (its clipped bounding box), by their number: one lane; the wave's 64
// lanes, up to 1024 turns; the whole grid of lightmap_owner_big_kernel.
constexpr uint32_t LIGHTMAP_LANE_MAX = 64;
constexpr uint32_t LIGHTMAP_WAVE_MAX = 65536;
constexpr uint32_t LIGHTMAP_THREADS = 256;       // texels per workgroup of the count, the record pass and the assembly
constexpr uint32_t LIGHTMAP_OWNER_BLOCKS = 2048;  // at most: 256 CUs x 8 workgroups, the rest by a grid stride
constexpr uint32_t LIGHTMAP_BIG_BLOCKS = 1024;    // 262144 threads: a triangle of the list gives each at least a quarter turn

// The mesh and the atlas as the owner pass and the record pass read them.
struct LightmapDev {
    const double* verts;    // nv * 3, f32 input already widened
    const uint32_t* idx;    // m * 3
    const double* uvs;      // m * 6
    const double* normals;  // m * 3: the triangles' unit normals from the host, flip applied
    uint32_t* owner;        // h * w
    uint32_t m, w, h;
};

// What the compaction leaves beside the workgroups' offsets.
struct LightmapCount {
    uint32_t n, big;  // the list's length; the triangles in the owner pass's list for the whole grid
};

// The list's arrays, written by the record pass at a texel's place in the list.
struct LightmapList {
    uint32_t* index;  // n
    double* points;   // n * 3
    double* normals;  // n * 3
    double* bary;     // n * 3
};

#if defined(__HIPCC__)
// COVERAGE's set-up of one triangle: its corners in texel space, area2 after the negation, whether it was negated, and its
// candidates x0 .. x1, y0 .. y1 (bw == 0: it covers nothing).
struct LightmapTri {
    double U0, V0, U1, V1, U2, V2, area2;
    bool negated;
    uint32_t x0, y0, bw, bh;
};

// The candidates along one axis: the integers x of 0 .. n - 1 with (double)(x + 1) >= lo && (double)x <= hi.  lo and hi are
// finite; the conversions are of values inside 0 .. n.
__device__ __forceinline__ void lightmap_span(double lo, double hi, uint32_t n, uint32_t& first, uint32_t& count) {
    const double dn = (double)n;
    first = 0u, count = 0u;
    if (!(hi >= 0.0) || !(lo <= dn)) return;
    first = lo <= 1.0 ? 0u : (uint32_t)__builtin_ceil(lo) - 1u;             // (1 < lo <= n: 1 .. n - 1)
    const uint32_t last = hi >= dn - 1.0 ? n - 1u : (uint32_t)__builtin_floor(hi);  // (0 <= hi < n - 1)
    if (first < n && last >= first) count = last - first + 1u;
}

__device__ __forceinline__ LightmapTri lightmap_setup(const LightmapDev& lm, uint32_t k) {
    const double* uv = lm.uvs + (size_t)k * 6u;
    const double W = (double)lm.w, H = (double)lm.h;
    LightmapTri t;
    t.U0 = uv[0] * W, t.V0 = uv[1] * H, t.U1 = uv[2] * W, t.V1 = uv[3] * H, t.U2 = uv[4] * W, t.V2 = uv[5] * H;
    t.area2 = (t.U1 - t.U0) * (t.V2 - t.V0) - (t.V1 - t.V0) * (t.U2 - t.U0);
    t.negated = t.area2 < 0.0;
    if (t.negated) t.area2 = -t.area2;
    t.x0 = t.y0 = t.bw = t.bh = 0u;
    const bool finite = __builtin_isfinite(t.U0) && __builtin_isfinite(t.V0) && __builtin_isfinite(t.U1) && __builtin_isfinite(t.V1) &&
                        __builtin_isfinite(t.U2) && __builtin_isfinite(t.V2);
    if (finite && __builtin_isfinite(t.area2) && t.area2 > 0.0) {
        const double umin = t.U0 < t.U1 ? (t.U0 < t.U2 ? t.U0 : t.U2) : (t.U1 < t.U2 ? t.U1 : t.U2);
        const double umax = t.U0 > t.U1 ? (t.U0 > t.U2 ? t.U0 : t.U2) : (t.U1 > t.U2 ? t.U1 : t.U2);
        const double vmin = t.V0 < t.V1 ? (t.V0 < t.V2 ? t.V0 : t.V2) : (t.V1 < t.V2 ? t.V1 : t.V2);
        const double vmax = t.V0 > t.V1 ? (t.V0 > t.V2 ? t.V0 : t.V2) : (t.V1 > t.V2 ? t.V1 : t.V2);
        lightmap_span(umin, umax, lm.w, t.x0, t.bw);
        lightmap_span(vmin, vmax, lm.h, t.y0, t.bh);
        if (t.bw == 0u || t.bh == 0u) t.bw = t.bh = 0u;
    }
    return t;
}

// The three edge functions at the centre of texel (x, y), negated with the triangle; does the triangle cover the texel?
__device__ __forceinline__ bool lightmap_covers(const LightmapTri& t, uint32_t x, uint32_t y, double& w1, double& w2) {
    const double px = (double)x + 0.5, py = (double)y + 0.5;
    double w0 = (t.U2 - t.U1) * (py - t.V1) - (t.V2 - t.V1) * (px - t.U1);
    w1 = (t.U0 - t.U2) * (py - t.V2) - (t.V0 - t.V2) * (px - t.U2);
    w2 = (t.U1 - t.U0) * (py - t.V0) - (t.V1 - t.V0) * (px - t.U0);
    if (t.negated) w0 = -w0, w1 = -w1, w2 = -w2;
    return w0 >= 0.0 && w1 >= 0.0 && w2 >= 0.0;
}
#endif

inline uint32_t lightmap_blocks(uint64_t texels) { return (uint32_t)((texels + LIGHTMAP_THREADS - 1u) / LIGHTMAP_THREADS); }

// owner = the lowest covering triangle per texel (the plane set to LIGHTMAP_NO_OWNER first, count zeroed).  big_list: m words.
hipError_t launch_lightmap_owner(const LightmapDev& lm, uint32_t* big_list, LightmapCount* count, hipStream_t stream);
// block_offsets (lightmap_blocks(w * h) words) = the owned texels before each workgroup's 256, count->n = their total
hipError_t launch_lightmap_compact(const LightmapDev& lm, uint32_t* block_offsets, LightmapCount* count, hipStream_t stream);
// the records of the owned texels at their places in the list
hipError_t launch_lightmap_records(const LightmapDev& lm, const uint32_t* block_offsets, const LightmapList& list, hipStream_t stream);
// ASSEMBLY's scatter: image (w * h * c) and valid (w * h) zeroed, then row i of values to texel index[i]
hipError_t launch_lightmap_scatter(const uint32_t* index, uint64_t n, const double* values, uint32_t c, uint64_t texels, double* image,
                                   uint8_t* valid, hipStream_t stream);
// one round of dilation from (image_in, valid_in) into (image_out, valid_out); *changed = 1 if a texel became valid
hipError_t launch_lightmap_dilate(const double* image_in, const uint8_t* valid_in, double* image_out, uint8_t* valid_out, uint32_t w,
                                  uint32_t h, uint32_t c, uint32_t* changed, hipStream_t stream);

}  // namespace rayrs
