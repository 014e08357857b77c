// features_host.hpp -- the host side of features.hip, shared by features_abi.cpp (rayrs_render_features,
// rayrs_image_denoise) and film_abi.cpp (rayrs_film_features, rayrs_film_denoise); and of guided.hip's filter, shared by
// guided_abi.cpp (rayrs_image_denoise_guided) and film_abi.cpp (rayrs_film_denoise_guided).
#pragma once
#include <cstdint>

#include "device_mem.hpp"
#include "feature_kernels.h"
#include "guided_kernels.h"
#include "scene_internal.hpp"

namespace rayrs {

// The five planes of a features pass on the device, in image order, and the traversal stacks' overflow strip.
struct FeatureBufs {
    DevBuf normal, albedo, depth, coverage, prim, spill;
};

// The refusals of a features pass that need no device: RAYRS_INVALID_ARG for samples = 0 or >= 2^30, a bad tile share,
// fast_traversal > 1, an empty image; RAYRS_UNSUPPORTED for an image side > 65535.
int features_check(const rayrs_camera* camera, uint32_t samples, uint32_t tile_rank, uint32_t tile_ranks, uint32_t fast_traversal);
// Clears the planes (+0, 0xffffffff) and runs the pass on the scene's device (already current), on the null stream.
int features_run(rayrs_scene* scene, const rayrs_camera* camera, uint32_t samples, uint64_t seed, uint32_t tile_rank,
                 uint32_t tile_ranks, uint32_t fast_traversal, FeatureBufs& b);
// Copies the wanted planes (null = not wanted) to the host; the object plane is numbered in insertion order there.
int features_download(const rayrs_scene* scene, const rayrs_camera* camera, const FeatureBufs& b, double* normal, double* albedo,
                      double* depth, double* coverage, uint32_t* object);
// levels outside 1 .. 16, or a k that is negative or not finite: RAYRS_INVALID_ARG
int denoise_check(uint32_t levels, double kn, double ka, double kz, double kc);
// `levels` launches on the null stream, ping-pong between `ping` and `pong` (grown here); level 0 reads d_color, which is
// not written.  The last level stores to *result (one of the two) in out_format.
int denoise_run(uint32_t w, uint32_t h, const double* d_color, const double* d_normal, const double* d_albedo, const double* d_depth,
                uint32_t levels, double kn, double ka, double kz, double kc, uint32_t out_format, DevBuf& ping, DevBuf& pong,
                void** result);

// The guided filter's working buffers: the two record frames, and the last level's colour and variance planes.
struct GuidedBufs {
    DevBuf ping, pong, color, variance;
};
// A pack and `levels` launches on the null stream: level 0 reads the records packed from d_color and d_variance (neither
// is written), the last level stores b.color in out_format and, with want_variance, b.variance.
int guided_run(uint32_t w, uint32_t h, const double* d_color, const double* d_variance, const double* d_normal, const double* d_albedo,
               const double* d_depth, uint32_t levels, double kn, double ka, double kz, double kv, uint32_t out_format,
               bool want_variance, GuidedBufs& b);

}  // namespace rayrs
