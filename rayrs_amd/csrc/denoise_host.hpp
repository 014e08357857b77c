// denoise_host.hpp -- the host side of denoise.hip's two a-trous filters, shared by denoise_abi.cpp (rayrs_image_denoise,
// rayrs_image_denoise_guided) and film_abi.cpp (rayrs_film_denoise, rayrs_film_denoise_guided).
#pragma once
#include <cstdint>

#include "denoise_kernels.h"
#include "device_mem.hpp"

namespace rayrs {

// What a filter reads, on the device; none of it is written.  variance = null: the feature-guided filter (k = kc); else the
// variance-guided one (k = kv).  A feature plane may be null: its term is left out.
struct DenoiseIn {
    uint32_t w, h;
    const double *color, *variance, *normal, *albedo, *depth;
};

// A filter's working buffers, grown on demand and shared by both filters (a frame is H * W * 3 doubles to the plain filter,
// H * W GuidedRec to the guided one): the two level frames, and the guided filter's last-level colour and variance planes.
struct DenoiseBufs {
    DevBuf frame[2], color, variance;
};

// levels outside 1 .. 16, or a k that is negative or not finite: RAYRS_INVALID_ARG
int denoise_check(uint32_t levels, double kn, double ka, double kz, double k);
// `levels` launches on the null stream (after a pack, guided); level l writes frame[l & 1] and reads the other one.  The
// last level stores the colour in out_format to *result -- its frame (plain) or b.color (guided) -- and, guided with
// want_variance, the variance to b.variance.
int denoise_run(const DenoiseIn& in, uint32_t levels, double kn, double ka, double kz, double k, uint32_t out_format,
                bool want_variance, DenoiseBufs& b, const void** result);

}  // namespace rayrs
