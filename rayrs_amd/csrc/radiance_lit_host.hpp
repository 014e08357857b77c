// radiance_lit_host.hpp -- what the three units of entry points that take a light list share (radiance_lit_abi.cpp: LIGHT SAMPLING,
// radiance_direct_abi.cpp: DIRECT LIGHTING, radiance_sky_abi.cpp: SKY SAMPLING): a call's description and its way from the refusals
// through the launches, all in radiance_lit_abi.cpp.  A call differs between the three in `direct` and `sky` alone.
#pragma once
#include "../../include/rayrs_hip.h"
#include "radiance_direct_kernels.h"
#include "radiance_lit_kernels.h"
#include "radiance_sky_table.h"
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
    bool sky;     // SKY SAMPLING (with direct): radiance_sky.hip's kernels, the sky one more light; an empty table is refused
};

// the four ray and point entry points, and the image form, of either unit
int lit_entry(rayrs_scene* scene, const LitCall& c, const double* a, const double* b, uint64_t n, double* radiance, uint32_t* queries,
              bool launch, void* hip_stream);
int lit_render(rayrs_scene* scene, const rayrs_camera* camera, const LitCall& c, double* out_rgb, uint32_t* queries);

// What the direct-lit films (film_abi.cpp, include/rayrs_hip.h DIRECT-LIT FILMS) take of that way, piece by piece: the list's
// refusals of the two groups (RAYRS_OK: none), the checked list as the table and as the slots the kernels take by value, and the
// scene's radiance scratch around a run of launches on `stream` (rd's thresholds, cursor, item sums, item counts and spill strip).
int lit_list_invalid(rayrs_scene* scene, const LitCall& c);
int lit_list_unsupported(rayrs_scene* scene, const LitCall& c);
LightsDev lights_resolve(rayrs_scene* scene, const LitCall& c);
LightSlotsDev direct_slots(rayrs_scene* scene, const LitCall& c);
int lit_scratch_begin(rayrs_scene* scene, const SceneDev& sc, hipStream_t stream, RadianceDev* rd);
int lit_scratch_end(rayrs_scene* scene, hipStream_t stream);

// The sky's table of the host scene's HDRI, built at the first call (radiance_sky_abi.cpp); `table` is a host pointer.
SkyDev sky_host_table(rayrs_scene* scene);
// T > 0.0 and finite: there is something to sample.
bool sky_table_usable(rayrs_scene* scene);
// The same with the device copy, uploaded at the first call (the scene's device is current).
int sky_device_table(rayrs_scene* scene, SkyDev* out);

}  // namespace rayrs
