// film_host.hpp -- a film's view as history_abi.cpp (rayrs_history_push_film) takes it: the frame, the noise plane, the
// per-tile sample counts and the features of the film as it stands, left on the device by film_abi.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/rayrs_hip.h"

namespace rayrs {

// Device pointers into the film's own buffers: valid until the film's next call, none of it written by the reader.
struct FilmView {
    rayrs_scene* scene;
    const rayrs_camera* camera;
    const double* color;     // what rayrs_film_read(RAYRS_OUT_F64) returns
    const double* variance;  // what rayrs_film_noise returns
    const uint32_t* tile_n;  // N_t per 8x8 tile of the frame, tiles_x in a row
    uint32_t tiles_x;
    const double *normal, *albedo, *depth, *coverage;  // the film's features
    const uint32_t* prim;    // ... the object plane as depth-first slots (features_download numbers it in insertion order)
};

// The refusals that need no device, as rayrs_film_denoise_guided has them: RAYRS_INVALID_ARG for a null or empty film, a
// film with tile_ranks > 1, feature_samples = 0 or >= 2^30.  *device = the film's.
int film_view_check(const rayrs_film* film, uint32_t feature_samples, int* device);
// Settles the film's scene, then makes the features (unless the film holds them), the frame and the noise plane on the
// null stream; marks (may be null): three events, recorded behind each of the three.
int film_view(rayrs_film* film, uint32_t feature_samples, FilmView* out, const hipEvent_t* marks);

}  // namespace rayrs
