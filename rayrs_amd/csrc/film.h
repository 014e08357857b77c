// film.h -- the progressive film's device records and the launch wrappers of film.hip
// (include/rayrs_hip.h rayrs_film_*).
#pragma once
#include <hip/hip_runtime.h>

#include "layout.h"

namespace rayrs {

// One record per pixel of the frame's 8x8 tiles, whoever renders them: the running sum of the pixel's chunk sums (x, y,
// z), and S1 and S2, the sum and the sum of squares of the channel sums y_k = (x_k + y_k) + z_k of its FULL chunks.
// 40 bytes, stored by tile as five planes of 64 doubles -- plane p of tile t begins at double (t * 5 + p) * 64 -- so
// that the 64 lanes of a wave, which hold the 64 pixels of one tile, read and write 512 contiguous bytes per plane.
constexpr uint32_t FILM_PLANES = 5;
constexpr uint32_t FILM_TILE_DOUBLES = FILM_PLANES * 64u;
constexpr uint32_t FILM_SX = 0, FILM_SY = 1, FILM_SZ = 2, FILM_S1 = 3, FILM_S2 = 4;

// A pass as the accumulate kernel sees it.
struct FilmPassDev {
    double* rec;           // the film's records
    uint32_t first;        // 1 = the film is empty: the pass's first chunk sum is ASSIGNED (resolve_kernel's k == 0); a pass
                           // over a tile list takes it per tile instead (TileRef::samples == 0)
    uint32_t full_chunks;  // chunks of the pass, counted from its first, that have all `chunk` samples (the others: only
                           // the last one of a pass that closes the film) and enter S1 and S2
    uint32_t* tile_n;      // N_t, the samples each tile of the frame holds: the pass writes its tiles' new counts
    // a pass over some of the share's tiles, each from its own N_t (film_compact_kernel's list), or null: every tile of
    // the share from RenderDev::sample0.  It becomes RenderDev::tile_list, n_list the pass's n_local_tiles.
    const TileRef* list;
    uint32_t n_list, pad;
};

struct FilmCounts {  // film_status_kernel's four counters, and the largest N_t among the share's tiles
    unsigned long long nan_pixels, neg_pixels, unconverged, nonfinite;
    unsigned int max_samples, pad;
};

struct FilmSelect {  // what film_compact_kernel leaves for the host: one of the two words is read back per pass
    uint32_t n_active;     // entries of the list
    uint32_t max_samples;  // the largest N_t among the share's tiles, before the pass
};

// Takes resolve_kernel's place behind a film pass's path rounds: adds the pass's chunk sums of the rank's tiles
// lt0 .. lt0 + n_lt - 1 (rp.partial, which starts at item rp.partial_item0) to the records, in chunk order.
hipError_t launch_film_accumulate(const CameraDev& cam, const RenderDev& rp, const FilmPassDev& fp, uint32_t lt0, uint32_t n_lt,
                                  hipStream_t stream);
// counts += the NaN / negative / unconverged / non-finite pixels among the share's tiles, each tile with its own
// M_t = tile_n[t] / c; tau2 = tau * tau
hipError_t launch_film_status(const CameraDev& cam, const TileShare& ts, const double* rec, const uint32_t* tile_n, uint32_t c,
                              double tau2, FilmCounts* counts, hipStream_t stream);
// out (W * H * 3, f32 or f64, row-major) = running sum * (1 / N_t); pixels of other ranks' tiles (N_t = 0) read as +0
hipError_t launch_film_read(const CameraDev& cam, uint32_t tiles_x, const double* rec, const uint32_t* tile_n, uint32_t out_format,
                            void* out, hipStream_t stream);
// The tiles of an adaptive pass (include/rayrs_hip.h rayrs_film_render_adaptive): flags[lt] = tile lt of the share has
// N_t + n <= cap and an in-image pixel that is unconverged at tau (all != 0: every tile of the share, whatever it
// holds); then list = the flagged tiles with their N_t in ascending tile order, and *sel.  flags: n_local_tiles words,
// list: n_local_tiles entries.
hipError_t launch_film_select(const CameraDev& cam, const TileShare& ts, const double* rec, const uint32_t* tile_n, uint32_t c,
                              uint32_t n, uint32_t cap, double tau2, uint32_t all, uint32_t* flags, TileRef* list, FilmSelect* sel,
                              hipStream_t stream);

}  // namespace rayrs
