// film_direct_kernels.h -- the direct-lit films (include/rayrs_hip.h DIRECT-LIT FILMS: rayrs_film_create_direct,
// rayrs_film_create_sky): the start a film pass gives the direct wave (and film_mesh.hip's group wave), what film_direct.hip's kernels are handed
// beside the waves' arguments, and their launch wrappers.  The scratch, the thresholds, the light table and the slots are the
// radiance queries' (radiance_kernels.h, radiance_lit_kernels.h, radiance_direct_kernels.h); the item numbering is the one
// film.hip's film_accumulate_kernel reads a pass's chunk sums by.
#pragma once
#include <hip/hip_runtime.h>

#include "layout.h"
#include "radiance_sky_kernels.h"

namespace rayrs {

// One launch of a pass: the pass's tiles lt0 .. lt0 + rd.n / 64 - 1 (local tiles of the share, or entries of the pass's list).
// RadianceDev carries the rest: n = the launch's tiles * 64, chunk = c, chunks = the pass's chunks per pixel, and the scratch.
struct FilmStartDev {
    TileShare share;            // the film's; n_local_tiles is the pass's tiles (the list's length under a list)
    const TileRef* tile_list;   // null: every tile of the share from sample0.  Else the pass's tiles, each from its own N_t
    uint32_t sample0, spp;      // the window: samples sample0 (or N_t) .. + spp - 1
    uint32_t lt0, pad;
};

// The pixel of item `item` of such a launch, (lt, k, pit) = (lt0 + item / (64 * chunks), (item / 64) % chunks, item % 64), and
// where its tile's window begins; false: the pixel is outside the share or the image (film_accumulate_kernel's own test).
#if defined(__HIPCC__)
__device__ __forceinline__ bool film_item_pixel(const FilmStartDev& fs, const CameraDev& cam, uint32_t chunks, uint32_t item, uint32_t& row,
                                                uint32_t& col, uint32_t& k, uint32_t& n_before) {
    const uint32_t pit = item & 63u, q = item >> 6;
    const uint32_t ltl = q / chunks;
    k = q - ltl * chunks;
    const uint32_t lt = fs.lt0 + ltl;
    const TilePixel own = tile_pixel(fs.share, lt, pit);
    row = own.row, col = own.col, n_before = fs.sample0;
    if (fs.tile_list != nullptr) {  // (an lt outside the pass reads entry 0, always there; in_share stays false)
        // (the entry in one 8-byte load: read word by word, the second word's load is moved behind a choice between its address and
        // a copy of sample0 on the stack, and the kernel would have a stack for that alone)
        const unsigned long long t = *reinterpret_cast<const unsigned long long*>(fs.tile_list + (own.in_share ? lt : 0u));
        const TilePixel listed = pixel_of_tile(fs.share, (uint32_t)t, pit, own.in_share);
        row = listed.row, col = listed.col, n_before = (uint32_t)(t >> 32);
    }
    return own.in_share && row < cam.H && col < cam.W;
}

// The film's start of radiance_direct_wave.h's and radiance_group_wave.h's waves.  A lane's `ray` is its pixel, row << 16 | col (a
// film's sides are below 65536); the RNG key and the primary ray are LIT_START_PIXEL's.
struct FilmStart {
    static constexpr int KIND = LIT_START_PIXEL;
    static constexpr bool SKIPS = true;
    const FilmStartDev& fs;  // (the kernel's argument)
    __device__ __forceinline__ unsigned long long n_items(const RadianceDev& rd) const { return (unsigned long long)rd.n * rd.chunks; }
    __device__ __forceinline__ bool take(const RadianceDev& rd, const CameraDev& cam, uint32_t item, uint32_t& ray, uint32_t& s,
                                         uint32_t& s_end) const {
        uint32_t row, col, k, n_before;
        if (!film_item_pixel(fs, cam, rd.chunks, item, row, col, k, n_before)) return false;
        ray = row << 16 | col;
        const uint32_t w_end = n_before + fs.spp;  // (at most 2^30 - 1: the pass rules)
        s = n_before + k * rd.chunk;
        s_end = s + rd.chunk < w_end ? s + rd.chunk : w_end;
        return true;
    }
    __device__ __forceinline__ void pixel(const RadianceDev&, const CameraDev&, uint32_t ray, uint32_t& row, uint32_t& col) const {
        row = ray >> 16, col = ray & 0xffffu;
    }
};
#endif

// What a pass's launches leave for the film: the closest-hit queries of its items, and its in-image pixels.
struct FilmDirectCounts {
    unsigned long long queries, pixels;
};

// film_direct_kernel (sky == nullptr) or film_sky_kernel on a grid of at most cu_count * RADIANCE_BLOCKS_PER_CU workgroups: the
// chunk sums of the launch's items into rd.partial, their query counts into rd.partial_queries, launch-local item numbering.
hipError_t launch_film_direct(bool compact, const SceneDev& sc, const RadianceDev& rd, const FilmStartDev& fs, const LightsDev& lights,
                              const LightSlotsDev& slots, const SkyDev* sky, const CameraDev& cam, int cu_count, hipStream_t stream);
// counts += the launch's items' query counts (rd.partial_queries; count_queries == 0: none were made) and its in-image pixels.
hipError_t launch_film_direct_count(const RadianceDev& rd, const FilmStartDev& fs, const CameraDev& cam, uint32_t count_queries,
                                    FilmDirectCounts* counts, hipStream_t stream);

}  // namespace rayrs
