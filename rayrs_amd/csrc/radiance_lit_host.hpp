// radiance_lit_host.hpp -- what the two units of entry points that take a light list share (radiance_lit_abi.cpp: LIGHT SAMPLING,
// radiance_direct_abi.cpp: DIRECT LIGHTING): a call's description and its way from the refusals through the launches, all in
// radiance_lit_abi.cpp.  A call differs between the two in `direct` alone.
#pragma once
#include "../../include/rayrs_hip.h"
#include "radiance_lit_kernels.h"
#include "scene_internal.hpp"

namespace rayrs {

// What a call asks for, beside its buffers.
struct LitCall {
    int start;  // LIT_START_*
    uint32_t samples, max_bounces, sample_chunk;
    double bias;
    uint64_t seed, index_base;
    uint32_t fast_traversal;
    const uint32_t* lights;
    uint32_t n_lights;
    bool direct;  // DIRECT LIGHTING: radiance_direct.hip's kernels, its overflow guard and its material rule
};

// the four ray and point entry points, and the image form, of either unit
int lit_entry(rayrs_scene* scene, const LitCall& c, const double* a, const double* b, uint64_t n, double* radiance, uint32_t* queries,
              bool launch, void* hip_stream);
int lit_render(rayrs_scene* scene, const rayrs_camera* camera, const LitCall& c, double* out_rgb, uint32_t* queries);

}  // namespace rayrs
