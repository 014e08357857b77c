// radiance_lit_abi.cpp -- the radiance queries with light sampling of include/rayrs_hip.h (LIGHT SAMPLING): the refusals, the
// light list resolved into the table the kernels take by value, a batch of rays, points or pixels through launches of
// radiance_lit.hip's kernels on the caller's stream, and the host forms around them.  The scratch, the staging, the stack strip
// and the lab's thresholds (rayrs_lab.h rayrs_lab_radiance_tuning) are the radiance queries' (radiance_abi.cpp).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "../../include/rayrs_hip.h"
#include "../../include/rayrs_numeric.h"
#include "radiance_direct_kernels.h"
#include "radiance_lit_host.hpp"
#include "radiance_lit_kernels.h"
#include "radiance_mesh_kernels.h"
#include "radiance_tree_kernels.h"
#include "radiance_sky_kernels.h"
#include "scene_internal.hpp"

namespace rayrs {

// The depth-first slot of every object (the inverse of flat.prim_object), made once.
const std::vector<uint32_t>& lit_object_prim(rayrs_scene* scene) {
    std::vector<uint32_t>& map = scene->lit.object_prim;
    const std::vector<uint32_t>& po = scene->flat.prim_object;
    if (map.size() != po.size()) {
        map.assign(po.size(), 0u);
        for (size_t p = 0; p < po.size(); p++) map[po[p]] = (uint32_t)p;
    }
    return map;
}

const uint32_t* prim_record(const rayrs_scene* scene, uint32_t p) {
    const uint32_t dw = scene->flat.compact ? PRIM_DWORDS_COMPACT : PRIM_DWORDS_FULL;
    return reinterpret_cast<const uint32_t*>(scene->flat.prim_bytes.data()) + (size_t)p * dw;
}
uint32_t lit_prim_tag(const rayrs_scene* scene, uint32_t p) {
    return prim_record(scene, p)[(scene->flat.compact ? PRIM_DWORDS_COMPACT : PRIM_DWORDS_FULL) - 1u];
}

namespace {

// DIRECT LIGHTING's material rule on a list whose indices are checked (true: refuse).  A listed object that emits must have a
// material whose scatter has no NoScatter path -- LambertianDiffuse, Reflect, Glass (material.rs: Refract and the Cook-Torrance
// family, Plastic's arm among them, can answer NoScatter, NoReflect always does): radiance() adds a hit's emission inside Scatter
// only (lib.rs:530-550), and the shadow sample credits emit() whole.
bool direct_list_unsupported(rayrs_scene* scene, const LitCall& c) {
    const std::vector<uint32_t>& map = lit_object_prim(scene);
    for (uint32_t k = 0; k < c.n_lights; k++) {
        const SurfaceDev& s = scene->surfaces[lit_prim_tag(scene, map[c.lights[k]]) >> 8];
        const bool dark = s.emit[0] == 0.0 && s.emit[1] == 0.0 && s.emit[2] == 0.0;
        const bool always_scatters = s.kind == RAYRS_MAT_LAMBERTIAN || s.kind == RAYRS_MAT_REFLECT || s.kind == RAYRS_MAT_GLASS;
        if (!dark && !always_scatters) return true;
    }
    return false;
}

}  // namespace

// The list as the depth-first slots a walk answers with (radiance_direct_kernels.h LightSlotsDev).
LightSlotsDev direct_slots(rayrs_scene* scene, const LitCall& c) {
    LightSlotsDev out;
    std::memset(&out, 0, sizeof(out));
    const std::vector<uint32_t>& map = lit_object_prim(scene);
    for (uint32_t k = 0; k < c.n_lights; k++) out.prim[k] = map[c.lights[k]];
    return out;
}

// lit_check's two pieces about the list, which the direct-lit films' creation takes as they are (film_abi.cpp): what of it is
// RAYRS_INVALID_ARG ...
int lit_list_invalid(rayrs_scene* scene, const LitCall& c) {
    if (c.n_lights > 0u && !c.lights) return RAYRS_INVALID_ARG;
    const size_t n_objects = scene->flat.prim_object.size();
    for (uint32_t k = 0; k < c.n_lights; k++)
        if (c.lights[k] >= n_objects) return RAYRS_INVALID_ARG;
    return RAYRS_OK;
}
// ... and, of a list that is not, what is RAYRS_UNSUPPORTED: too many lights, a triangle, DIRECT LIGHTING's material rule, and
// SKY SAMPLING's empty table (nothing to sample).
int lit_list_unsupported(rayrs_scene* scene, const LitCall& c) {
    if (c.n_lights > RAYRS_MAX_LIGHTS) return RAYRS_UNSUPPORTED;
    if (c.n_lights > 0u) {
        const std::vector<uint32_t>& map = lit_object_prim(scene);
        for (uint32_t k = 0; k < c.n_lights; k++)
            if ((lit_prim_tag(scene, map[c.lights[k]]) & 3u) == PRIM_TRIANGLE) return RAYRS_UNSUPPORTED;
        if (c.direct && direct_list_unsupported(scene, c)) return RAYRS_UNSUPPORTED;
    }
    if (c.sky && !sky_table_usable(scene)) return RAYRS_UNSUPPORTED;
    return RAYRS_OK;
}

namespace {

// The refusals that need no device, in the header's order: RADIANCE QUERY's with the list's among them.  `extra_invalid` and
// `extra_unsupported` are what the image form adds to the two groups (the camera's).  A direct call can make 2 * max_bounces + 1
// queries per path, and has its material rule.
int lit_check(rayrs_scene* scene, const void* a, const void* b, const void* radiance, const void* queries, const LitCall& c,
              bool extra_invalid = false, bool extra_unsupported = false) {
    if (!scene || !a || !b || (!radiance && !queries)) return RAYRS_INVALID_ARG;
    if (c.samples == 0u || c.fast_traversal > 1u || extra_invalid) return RAYRS_INVALID_ARG;
    RAYRS_TRY(lit_list_invalid(scene, c));
    if (c.mesh && c.mesh->scene != scene) return RAYRS_INVALID_ARG;
    if (c.samples > SLOT_SAMPLE_MASK || c.max_bounces > 8000u || extra_unsupported) return RAYRS_UNSUPPORTED;
    const uint64_t path_queries = c.direct ? 2ull * c.max_bounces + 1u : c.max_bounces;
    if ((uint64_t)c.samples * path_queries >= (1ull << 32)) return RAYRS_UNSUPPORTED;
    if (radiance_chunks(c.samples, c.sample_chunk) > RADIANCE_LAUNCH_ITEMS) return RAYRS_UNSUPPORTED;
    RAYRS_TRY(lit_list_unsupported(scene, c));
    if (scene->device < 0) return RAYRS_NO_DEVICE;
    return RAYRS_OK;
}

}  // namespace

// The table of a checked list (radiance_lit_kernels.h LightDev): the primitive record's f64 values as they are, and the two
// values a light's sample and density read on top, each one correctly rounded operation of the header's.
LightsDev lights_resolve(rayrs_scene* scene, const LitCall& c) {
    LightsDev out;
    std::memset(&out, 0, sizeof(out));
    out.n = c.n_lights;
    if (c.n_lights == 0u) return out;
    const std::vector<uint32_t>& map = lit_object_prim(scene);
    for (uint32_t k = 0; k < c.n_lights; k++) {
        const uint32_t p = map[c.lights[k]];
        const uint32_t tag = lit_prim_tag(scene, p);
        double v[5] = {0, 0, 0, 0, 0};
        std::memcpy(v, prim_record(scene, p), ((tag & 3u) == PRIM_SPHERE ? 4u : 5u) * sizeof(double));
        LightDev& L = out.light[k];
        L.kind = tag & 3u, L.axis = (tag >> 2) & 7u;
        if (L.kind == PRIM_SPHERE) {
            L.v[0] = v[0], L.v[1] = v[1], L.v[2] = v[2], L.v[3] = v[3];
            L.v[4] = std::sqrt(v[0]);          // radius2.sqrt()
            L.v[5] = (4.0 * RR_PI) * v[0];     // 4. * PI * radius2
        } else {
            L.v[0] = v[0], L.v[1] = v[1], L.v[2] = v[2], L.v[3] = v[3], L.v[4] = v[4];
            L.v[5] = (v[1] - v[0]) * (v[3] - v[2]);
        }
    }
    return out;
}

// What every launch on the scene's radiance scratch begins with: the scratch and the stack strip reserved, `stream` made to wait
// for the last launch that used them (the queries' ordering rule), and rd's thresholds, cursor, item sums, item query counts and
// spill strip filled in.  lit_scratch_end, behind the last launch, records the event the next user waits for.
int lit_scratch_begin(rayrs_scene* scene, const SceneDev& sc, hipStream_t stream, RadianceDev* rd) {
    rayrs_scene::Queries& strip = scene->queries;
    rayrs_scene::Radiance& own = scene->radiance;
    if (sc.stack_depth > sc.stack_lds) HIP_TRY(strip.d_stack_spill.reserve(stack_spill_words(sc, QUERY_LAUNCH_RAYS) * sizeof(uint32_t)));
    HIP_TRY(own.d_scratch.reserve(RADIANCE_SCRATCH_BYTES));
    if (!strip.has_event) {
        HIP_TRY(strip.ev_done.create());
        strip.has_event = true;
    }
    if (strip.strip_in_use) HIP_TRY(hipStreamWaitEvent(stream, strip.ev_done, 0));
    rd->refill_below = own.refill_below ? own.refill_below : RADIANCE_REFILL_BELOW;
    rd->shade_at = own.shade_at ? own.shade_at : RADIANCE_SHADE_AT;
    rd->leaf_min = own.leaf_min ? own.leaf_min : RADIANCE_LEAF_MIN;
    char* scratch = own.d_scratch.as<char>();
    rd->cursor = reinterpret_cast<unsigned long long*>(scratch);
    rd->partial = reinterpret_cast<double*>(scratch + RADIANCE_CURSOR_BYTES);
    rd->partial_queries = reinterpret_cast<uint32_t*>(scratch + RADIANCE_CURSOR_BYTES + RADIANCE_LAUNCH_ITEMS * 24u);
    rd->spill = strip.d_stack_spill.as<uint32_t>();
    return RAYRS_OK;
}
int lit_scratch_end(rayrs_scene* scene, hipStream_t stream) {
    HIP_TRY(hipEventRecord(scene->queries.ev_done, stream));
    scene->queries.strip_in_use = true;
    return RAYRS_OK;
}

namespace {

// The batch, whole rays of at most RADIANCE_LAUNCH_ITEMS items per launch, all on `stream`, as radiance_abi.cpp's
// radiance_enqueue: the same scratch, the same strip and the same ordering rule.  LIT_START_PIXEL: a and b are null and the
// rays are the camera's pixels index_base + i.
int lit_enqueue(rayrs_scene* scene, const LitCall& c, const SceneDev& sc, const LightsDev& lights, const CameraDev& cam, const double* a,
                const double* b, uint64_t n, double* radiance, uint32_t* queries, hipStream_t stream) {
    SkyDev sky;
    std::memset(&sky, 0, sizeof(sky));
    if (c.sky) RAYRS_TRY(sky_device_table(scene, &sky));  // (uploaded by the scene's first sky call, then kept)
    MeshDev mesh;
    std::memset(&mesh, 0, sizeof(mesh));
    const bool grouped = c.mesh && c.mesh->n != 0u;  // (an empty group: DIRECT LIGHTING's call, or SKY SAMPLING's)
    const bool treed = grouped && c.mesh->tree;  // LIGHT TREE: the group's triangles are chosen by its tree
    TreeDev tree;
    std::memset(&tree, 0, sizeof(tree));
    if (treed) RAYRS_TRY(tree_device_table(c.mesh, &tree));
    else if (grouped) RAYRS_TRY(mesh_device_table(c.mesh, &mesh));  // (uploaded by the handle's first call, then kept)
    if (c.max_bounces == 0u) {  // the loop runs no turn: +0 and no query, whatever the scene
        if (radiance) HIP_TRY(hipMemsetAsync(radiance, 0, n * 3u * sizeof(double), stream));
        if (queries) HIP_TRY(hipMemsetAsync(queries, 0, n * sizeof(uint32_t), stream));
        return RAYRS_OK;
    }
    LightSlotsDev slots;
    std::memset(&slots, 0, sizeof(slots));
    if (c.direct) slots = direct_slots(scene, c);
    RadianceDev rd;
    std::memset(&rd, 0, sizeof(rd));
    RAYRS_TRY(lit_scratch_begin(scene, sc, stream, &rd));
    rd.samples = c.samples, rd.max_bounces = c.max_bounces, rd.irradiance = c.start == LIT_START_POINT ? 1u : 0u;
    rd.chunk = radiance_chunk(c.samples, c.sample_chunk), rd.chunks = radiance_chunks(c.samples, c.sample_chunk);
    rd.seed = c.seed, rd.bias = c.bias;
    const uint64_t per_launch = RADIANCE_LAUNCH_ITEMS / rd.chunks;  // (>= 1: lit_check)
    for (uint64_t base = 0; base < n; base += per_launch) {
        rd.n = (uint32_t)(n - base < per_launch ? n - base : per_launch);
        rd.index_base = c.index_base + base;
        rd.a = a ? a + base * 3u : nullptr, rd.b = b ? b + base * 3u : nullptr;
        rd.radiance = radiance ? radiance + base * 3u : nullptr;
        rd.queries = queries ? queries + base : nullptr;
        HIP_TRY(hipMemsetAsync(rd.cursor, 0, sizeof(unsigned long long), stream));
        if (treed) HIP_TRY(launch_radiance_tree(scene->flat.compact, sc, rd, lights, slots, tree, sky, c.sky, cam, c.start, scene->cu_count, stream));
        else if (grouped) HIP_TRY(launch_radiance_mesh(scene->flat.compact, sc, rd, lights, slots, mesh, sky, c.sky, cam, c.start, scene->cu_count, stream));
        else if (c.sky) HIP_TRY(launch_radiance_sky(scene->flat.compact, sc, rd, lights, slots, sky, cam, c.start, scene->cu_count, stream));
        else if (c.direct) HIP_TRY(launch_radiance_direct(scene->flat.compact, sc, rd, lights, slots, cam, c.start, scene->cu_count, stream));
        else HIP_TRY(launch_radiance_lit(scene->flat.compact, sc, rd, lights, cam, c.start, scene->cu_count, stream));
    }
    return lit_scratch_end(scene, stream);
}

// The host form: upload (rays and points), launch on the null stream, wait, download.
int lit_host(rayrs_scene* scene, const LitCall& c, const SceneDev& sc, const LightsDev& lights, const CameraDev& cam, const double* a,
             const double* b, uint64_t n, double* radiance, uint32_t* queries) {
    rayrs_scene::Radiance& own = scene->radiance;
    if (a) HIP_TRY(own.d_a.upload(a, n * 3u * sizeof(double)));
    if (b) HIP_TRY(own.d_b.upload(b, n * 3u * sizeof(double)));
    if (radiance) HIP_TRY(own.d_radiance.reserve(n * 3u * sizeof(double)));
    if (queries) HIP_TRY(own.d_queries.reserve(n * sizeof(uint32_t)));
    RAYRS_TRY(lit_enqueue(scene, c, sc, lights, cam, a ? own.d_a.as<double>() : nullptr, b ? own.d_b.as<double>() : nullptr, n,
                          radiance ? own.d_radiance.as<double>() : nullptr, queries ? own.d_queries.as<uint32_t>() : nullptr, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    if (radiance) HIP_TRY(own.d_radiance.download(radiance, n * 3u * sizeof(double)));
    if (queries) HIP_TRY(own.d_queries.download(queries, n * sizeof(uint32_t)));
    return RAYRS_OK;
}

}  // namespace

int lit_entry(rayrs_scene* scene, const LitCall& c, const double* a, const double* b, uint64_t n, double* radiance, uint32_t* queries,
              bool launch, void* hip_stream) {
    RAYRS_TRY(lit_check(scene, a, b, radiance, queries, c));
    if (n == 0u) return RAYRS_OK;
    const LightsDev lights = lights_resolve(scene, c);
    CameraDev cam;
    std::memset(&cam, 0, sizeof(cam));
    HIP_TRY(hipSetDevice(scene->device));
    const SceneDev sc = make_scene_dev(scene, c.fast_traversal == 0u);
    if (!launch) return lit_host(scene, c, sc, lights, cam, a, b, n, radiance, queries);
    return lit_enqueue(scene, c, sc, lights, cam, a, b, n, radiance, queries, reinterpret_cast<hipStream_t>(hip_stream));
}

int lit_render(rayrs_scene* scene, const rayrs_camera* camera, const LitCall& c, double* out_rgb, uint32_t* queries) {
    // (the camera's refusals are FEATURES', as rayrs_render_ao's: an empty image with the arguments, a side above 65535 with the sizes)
    const bool no_image = camera && (camera->x_pixels == 0u || camera->y_pixels == 0u);
    const bool too_wide = camera && (camera->x_pixels > 65535u || camera->y_pixels > 65535u);
    RAYRS_TRY(lit_check(scene, camera, out_rgb, out_rgb, queries, c, no_image, too_wide));
    RAYRS_TRY(scene_settle(scene));
    const LightsDev table = lights_resolve(scene, c);
    const FrameWalk walk = frame_walk(scene, camera, c.fast_traversal);  // the walk a render with these settings takes
    const SceneDev sc = make_scene_dev(scene, walk.exact || walk.use_local);
    const CameraDev cam = make_camera_dev(camera);
    const uint64_t npix = (uint64_t)camera->x_pixels * camera->y_pixels;
    return lit_host(scene, c, sc, table, cam, nullptr, nullptr, npix, out_rgb, queries);
}

}  // namespace rayrs

using namespace rayrs;

extern "C" {

int rayrs_scene_radiance_lit(rayrs_scene* scene, const double* origin, const double* direction, uint64_t n, uint32_t samples,
                             uint32_t max_bounces, uint32_t sample_chunk, uint64_t seed, uint64_t index_base, uint32_t fast_traversal,
                             const uint32_t* lights, uint32_t n_lights, double* radiance, uint32_t* queries) {
    RAYRS_GUARDED({
    return lit_entry(scene, LitCall{LIT_START_RAY, samples, max_bounces, sample_chunk, 0.0, seed, index_base, fast_traversal, lights, n_lights},
                     origin, direction, n, radiance, queries, false, nullptr);
    })
}

int rayrs_scene_radiance_lit_launch(rayrs_scene* scene, const double* origin, const double* direction, uint64_t n, uint32_t samples,
                                    uint32_t max_bounces, uint32_t sample_chunk, uint64_t seed, uint64_t index_base,
                                    uint32_t fast_traversal, const uint32_t* lights, uint32_t n_lights, double* radiance,
                                    uint32_t* queries, void* hip_stream) {
    RAYRS_GUARDED({
    return lit_entry(scene, LitCall{LIT_START_RAY, samples, max_bounces, sample_chunk, 0.0, seed, index_base, fast_traversal, lights, n_lights},
                     origin, direction, n, radiance, queries, true, hip_stream);
    })
}

int rayrs_scene_irradiance_lit(rayrs_scene* scene, const double* position, const double* normal, uint64_t n, uint32_t samples,
                               uint32_t max_bounces, uint32_t sample_chunk, double bias, uint64_t seed, uint64_t index_base,
                               uint32_t fast_traversal, const uint32_t* lights, uint32_t n_lights, double* radiance, uint32_t* queries) {
    RAYRS_GUARDED({
    return lit_entry(scene, LitCall{LIT_START_POINT, samples, max_bounces, sample_chunk, bias, seed, index_base, fast_traversal, lights, n_lights},
                     position, normal, n, radiance, queries, false, nullptr);
    })
}

int rayrs_scene_irradiance_lit_launch(rayrs_scene* scene, const double* position, const double* normal, uint64_t n, uint32_t samples,
                                      uint32_t max_bounces, uint32_t sample_chunk, double bias, uint64_t seed, uint64_t index_base,
                                      uint32_t fast_traversal, const uint32_t* lights, uint32_t n_lights, double* radiance,
                                      uint32_t* queries, void* hip_stream) {
    RAYRS_GUARDED({
    return lit_entry(scene, LitCall{LIT_START_POINT, samples, max_bounces, sample_chunk, bias, seed, index_base, fast_traversal, lights, n_lights},
                     position, normal, n, radiance, queries, true, hip_stream);
    })
}

int rayrs_render_lit(rayrs_scene* scene, const rayrs_camera* camera, uint64_t seed, uint32_t samples, uint32_t max_bounces,
                     uint32_t sample_chunk, uint32_t fast_traversal, const uint32_t* lights, uint32_t n_lights, double* out_rgb,
                     uint32_t* queries) {
    RAYRS_GUARDED({
    return lit_render(scene, camera, LitCall{LIT_START_PIXEL, samples, max_bounces, sample_chunk, 0.0, seed, 0u, fast_traversal, lights, n_lights},
                      out_rgb, queries);
    })
}

}  // extern "C"
