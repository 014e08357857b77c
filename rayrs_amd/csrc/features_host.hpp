// features_host.hpp -- the host side of features.hip, shared by features_abi.cpp (rayrs_render_features) and film_abi.cpp
// (rayrs_film_features and the film's two filters).
#pragma once
#include <cstdint>

#include "device_mem.hpp"
#include "feature_kernels.h"
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

}  // namespace rayrs
