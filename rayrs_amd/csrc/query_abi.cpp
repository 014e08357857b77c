// query_abi.cpp -- ray queries of include/rayrs_hip.h (RAY QUERIES): the refusals, a batch of caller rays through launches
// of query.hip's kernels on the caller's stream, the host forms around them (upload, launch, wait, download), and the lab's
// step count (rayrs_lab.h rayrs_lab_query_steps).
#include <hip/hip_runtime.h>

#include <cstring>
#include <initializer_list>

#include "../../include/rayrs_hip.h"
#include "query_kernels.h"
#include "scene_internal.hpp"

using namespace rayrs;

namespace {

// The refusals that need no device, in the header's order; `required` are the call's buffers that may not be NULL.
int query_check(const rayrs_scene* scene, std::initializer_list<const void*> required, uint32_t fast_traversal) {
    if (!scene) return RAYRS_INVALID_ARG;
    for (const void* p : required)
        if (!p) return RAYRS_INVALID_ARG;
    if (fast_traversal > 1u) return RAYRS_INVALID_ARG;
    if (scene->device < 0) return RAYRS_NO_DEVICE;
    return RAYRS_OK;
}

// The batch, at most QUERY_LAUNCH_RAYS rays per launch, all on `stream`: `q` holds the whole batch's pointers, which move
// on from launch to launch.  fast_traversal is taken as asked (there is no camera for the camera rule to look at).  The
// launches of one batch follow one another on the stream and share the stack strip; a batch on another stream waits (on the
// device) for the strip's last user.
int query_enqueue(rayrs_scene* scene, bool occlusion, uint32_t fast_traversal, uint64_t n, QueryDev q, hipStream_t stream) {
    const SceneDev sc = make_scene_dev(scene, fast_traversal == 0u);
    rayrs_scene::Queries& own = scene->queries;
    const bool spills = sc.stack_depth > sc.stack_lds;
    if (spills) {
        HIP_TRY(own.d_stack_spill.reserve(stack_spill_words(sc, QUERY_LAUNCH_RAYS) * sizeof(uint32_t)));
        if (!own.has_event) {
            HIP_TRY(own.ev_done.create());
            own.has_event = true;
        }
        if (own.strip_in_use) HIP_TRY(hipStreamWaitEvent(stream, own.ev_done, 0));
    }
    q.spill = own.d_stack_spill.as<uint32_t>();
    for (uint64_t base = 0; base < n; base += QUERY_LAUNCH_RAYS) {
        QueryDev part = q;
        part.n = (uint32_t)(n - base < QUERY_LAUNCH_RAYS ? n - base : QUERY_LAUNCH_RAYS);
        part.origin = q.origin + base * 3u, part.direction = q.direction + base * 3u;
        if (occlusion) {
            part.t_max = q.t_max ? q.t_max + base : nullptr;
            part.occluded = q.occluded + base;
            part.steps = q.steps ? q.steps + base : nullptr;
            HIP_TRY(launch_query_occluded(scene->flat.compact, sc, part, stream));
        } else {
            part.t = q.t + base, part.object = q.object + base;
            part.normal = q.normal ? q.normal + base * 3u : nullptr;
            HIP_TRY(launch_query_intersect(scene->flat.compact, sc, part, stream));
        }
    }
    if (spills) {
        HIP_TRY(hipEventRecord(own.ev_done, stream));
        own.strip_in_use = true;
    }
    return RAYRS_OK;
}

int intersect_launch(rayrs_scene* scene, const double* origin, const double* direction, uint64_t n, uint32_t fast_traversal,
                     double* t, uint32_t* object, double* normal, hipStream_t stream) {
    QueryDev q;
    std::memset(&q, 0, sizeof(q));
    RAYRS_TRY(scene_prim_object(scene, &q.prim_object));
    q.n_prims = (uint32_t)scene->flat.prim_object.size();
    q.origin = origin, q.direction = direction;
    q.t = t, q.object = object, q.normal = normal;
    return query_enqueue(scene, false, fast_traversal, n, q, stream);
}

int occluded_launch(rayrs_scene* scene, const double* origin, const double* direction, const double* t_max, uint64_t n,
                    uint32_t fast_traversal, uint8_t* occluded, hipStream_t stream, uint32_t* steps = nullptr) {
    QueryDev q;
    std::memset(&q, 0, sizeof(q));
    q.origin = origin, q.direction = direction, q.t_max = t_max;
    q.occluded = occluded, q.steps = steps;
    return query_enqueue(scene, true, fast_traversal, n, q, stream);
}

// The occlusion query's host form -- upload, launch on the null stream, wait, download -- and the lab's with `steps` (which go
// through the closest-hit form's object buffer: a word per ray).
int occluded_host(rayrs_scene* scene, const double* origin, const double* direction, const double* t_max, uint64_t n,
                  uint32_t fast_traversal, uint8_t* occluded, uint32_t* steps) {
    HIP_TRY(hipSetDevice(scene->device));
    rayrs_scene::Queries& own = scene->queries;
    HIP_TRY(own.d_origin.upload(origin, n * 3u * sizeof(double)));
    HIP_TRY(own.d_direction.upload(direction, n * 3u * sizeof(double)));
    if (t_max) HIP_TRY(own.d_t_max.upload(t_max, n * sizeof(double)));
    HIP_TRY(own.d_occluded.reserve(n));
    if (steps) HIP_TRY(own.d_object.reserve(n * sizeof(uint32_t)));
    RAYRS_TRY(occluded_launch(scene, own.d_origin.as<double>(), own.d_direction.as<double>(), t_max ? own.d_t_max.as<double>() : nullptr, n,
                              fast_traversal, own.d_occluded.as<uint8_t>(), nullptr, steps ? own.d_object.as<uint32_t>() : nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(own.d_occluded.download(occluded, n));
    if (steps) HIP_TRY(own.d_object.download(steps, n * sizeof(uint32_t)));
    return RAYRS_OK;
}

}  // namespace

extern "C" {

int rayrs_scene_intersect_launch(rayrs_scene* scene, const double* origin, const double* direction, uint64_t n,
                                 uint32_t fast_traversal, double* t, uint32_t* object, double* normal, void* hip_stream) {
    RAYRS_GUARDED({
    RAYRS_TRY(query_check(scene, {origin, direction, t, object}, fast_traversal));
    if (n == 0u) return RAYRS_OK;
    HIP_TRY(hipSetDevice(scene->device));
    return intersect_launch(scene, origin, direction, n, fast_traversal, t, object, normal, reinterpret_cast<hipStream_t>(hip_stream));
    })
}

int rayrs_scene_occluded_launch(rayrs_scene* scene, const double* origin, const double* direction, const double* t_max, uint64_t n,
                                uint32_t fast_traversal, uint8_t* occluded, void* hip_stream) {
    RAYRS_GUARDED({
    RAYRS_TRY(query_check(scene, {origin, direction, occluded}, fast_traversal));
    if (n == 0u) return RAYRS_OK;
    HIP_TRY(hipSetDevice(scene->device));
    return occluded_launch(scene, origin, direction, t_max, n, fast_traversal, occluded, reinterpret_cast<hipStream_t>(hip_stream));
    })
}

int rayrs_scene_intersect(rayrs_scene* scene, const double* origin, const double* direction, uint64_t n, uint32_t fast_traversal,
                          double* t, uint32_t* object, double* normal) {
    RAYRS_GUARDED({
    RAYRS_TRY(query_check(scene, {origin, direction, t, object}, fast_traversal));
    if (n == 0u) return RAYRS_OK;
    HIP_TRY(hipSetDevice(scene->device));
    rayrs_scene::Queries& own = scene->queries;
    HIP_TRY(own.d_origin.upload(origin, n * 3u * sizeof(double)));
    HIP_TRY(own.d_direction.upload(direction, n * 3u * sizeof(double)));
    HIP_TRY(own.d_t.reserve(n * sizeof(double)));
    HIP_TRY(own.d_object.reserve(n * sizeof(uint32_t)));
    if (normal) HIP_TRY(own.d_normal.reserve(n * 3u * sizeof(double)));
    RAYRS_TRY(intersect_launch(scene, own.d_origin.as<double>(), own.d_direction.as<double>(), n, fast_traversal, own.d_t.as<double>(),
                               own.d_object.as<uint32_t>(), normal ? own.d_normal.as<double>() : nullptr, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(own.d_t.download(t, n * sizeof(double)));
    HIP_TRY(own.d_object.download(object, n * sizeof(uint32_t)));
    if (normal) HIP_TRY(own.d_normal.download(normal, n * 3u * sizeof(double)));
    return RAYRS_OK;
    })
}

int rayrs_scene_occluded(rayrs_scene* scene, const double* origin, const double* direction, const double* t_max, uint64_t n,
                         uint32_t fast_traversal, uint8_t* occluded) {
    RAYRS_GUARDED({
    RAYRS_TRY(query_check(scene, {origin, direction, occluded}, fast_traversal));
    if (n == 0u) return RAYRS_OK;
    return occluded_host(scene, origin, direction, t_max, n, fast_traversal, occluded, nullptr);
    })
}

int rayrs_lab_query_steps(rayrs_scene* scene, const double* origin, const double* direction, const double* t_max, uint64_t n,
                          uint32_t fast_traversal, uint8_t* occluded, uint32_t* steps) {
    RAYRS_GUARDED({
    RAYRS_TRY(query_check(scene, {origin, direction, occluded, steps}, fast_traversal));
    if (n == 0u) return RAYRS_OK;
    return occluded_host(scene, origin, direction, t_max, n, fast_traversal, occluded, steps);
    })
}

}  // extern "C"
