// radiance_wave_parts.h -- what is the same text in the waves of radiance.hip, radiance_lit.hip, radiance_direct_wave.h and
// radiance_group_wave.h, written once: the queries' start (which item is which ray and chunk), the start of a sample before the
// lighting has its say, and the body of the four resolve kernels, which keep their names and their units.
#pragma once
#include "device_path.h"
#include "radiance_lit_kernels.h"
#include "radiance_probe_table.h"

namespace rayrs {

// Who starts the wave's paths: which items a launch has, what item `item` is, and the pixel of a LIT_START_PIXEL ray.  This one
// is the queries': item = ray * chunks + chunk of the rays 0 .. rd.n - 1, every item taken; a pixel is index_base + ray in image
// order.  KIND is the LIT_START_* the sample's start is made by; SKIPS says whether take() can turn an item down.
template <int START>
struct QueryStart {
    static constexpr int KIND = START;
    static constexpr bool SKIPS = false;
    RR_DEV unsigned long long n_items(const RadianceDev& rd) const { return (unsigned long long)rd.n * rd.chunks; }
    RR_DEV bool take(const RadianceDev& rd, const CameraDev&, uint32_t item, uint32_t& ray, uint32_t& s, uint32_t& s_end) const {
        ray = item / rd.chunks;
        s = (item - ray * rd.chunks) * rd.chunk;
        s_end = rd.samples - s < rd.chunk ? rd.samples : s + rd.chunk;
        return true;
    }
    RR_DEV void pixel(const RadianceDev& rd, const CameraDev& cam, uint32_t ray, uint32_t& row, uint32_t& col) const {
        const uint32_t pix = (uint32_t)rd.index_base + ray;  // (the image's pixels: below 2^32)
        row = pix / cam.W, col = pix - row * cam.W;
    }
};

// What every sample starts from: its RNG and a ray.  LIT_START_PIXEL: sample_key and the camera's sample_ray on draws 0 and 1.
// LIT_START_RAY: the caller's ray, draw 0 next.  LIT_START_POINT: o is the point moved along its normal by the bias and d is the
// NORMAL, draw 0 next -- the first direction is the lighting's to make (device_path.h cosine_direction, or its own operation at
// the point).  LIT_START_PROBE: o is the probe's point, d the direction of draws 0 and 1 (radiance_probe_table.h), draw 2 next.
// By value: handed out by reference, the six doubles go through the stack in the point instances.
struct SampleStart {
    Rng rng;
    V3 o, d;
};
template <class START>
RR_DEV SampleStart sample_start(const START& start, const RadianceDev& rd, const CameraDev& cam, uint32_t ray, uint32_t s) {
    Rng rng;
    V3 o, d;
    if (START::KIND == LIT_START_PIXEL) {
        uint32_t row, col;
        start.pixel(rd, cam, ray, row, col);
        rng = Rng{sample_key(rd.seed, cam, row, col, s), 0};
        sample_ray(cam, row, col, rng, o, d);
        return SampleStart{rng, o, d};
    }
    const double* pa = rd.a + (size_t)ray * 3u;
    if (START::KIND == LIT_START_PROBE) {  // (rd.b is not read: a probe has no second array)
        rng = Rng{rr_path_key(rd.seed, rd.index_base + ray, (uint64_t)s), 0};
        const double u1 = rng.next();
        const double u2 = rng.next();
        double w[3];
        probe_direction(u1, u2, w);
        return SampleStart{rng, mk(pa[0], pa[1], pa[2]), mk(w[0], w[1], w[2])};
    }
    const double* pb = rd.b + (size_t)ray * 3u;
    const V3 a = mk(pa[0], pa[1], pa[2]), b = mk(pb[0], pb[1], pb[2]);
    rng = Rng{rr_path_key(rd.seed, rd.index_base + ray, (uint64_t)s), 0};
    if (START::KIND == LIT_START_POINT) o = v_add(a, v_scale(b, rd.bias)), d = b;
    else o = a, d = b;
    return SampleStart{rng, o, d};
}


// A ray's chunk sums added in chunk order (the first assigned), scaled by the reciprocal of S, and its query counts added:
// one thread per ray.
RR_DEV void radiance_resolve(const RadianceDev& rd) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= rd.n) return;
    const double* p = rd.partial + (size_t)i * rd.chunks * 3u;
    const uint32_t* pq = rd.partial_queries + (size_t)i * rd.chunks;
    V3 sum = mk(p[0], p[1], p[2]);
    uint32_t q = pq[0];
    for (uint32_t k = 1; k < rd.chunks; k++) {
        sum = v_add(sum, mk(p[3u * k], p[3u * k + 1u], p[3u * k + 2u]));
        q += pq[k];
    }
    const double inv = 1.0 / (double)rd.samples;
    if (rd.radiance != nullptr) {
        double* dst = rd.radiance + (size_t)i * 3u;
        dst[0] = sum.x * inv, dst[1] = sum.y * inv, dst[2] = sum.z * inv;
    }
    if (rd.queries != nullptr) rd.queries[i] = q;
}

// One of those kernels behind a launch's wave kernel, on the same stream.
inline hipError_t launch_radiance_resolve(void (*kernel)(RadianceDev), const RadianceDev& rd, hipStream_t stream) {
    hipLaunchKernelGGL(kernel, dim3((rd.n + 255u) / 256u), dim3(256), 0, stream, rd);
    return hipGetLastError();
}

}  // namespace rayrs
