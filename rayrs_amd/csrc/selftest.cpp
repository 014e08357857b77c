// selftest.cpp -- the device self tests declared in rayrs_selftest.h (tests/ only): single device functions and the
// traversal kernel run on caller data, outside a render.
#include <cstring>
#include <vector>

#include "kernels.h"
#include "rayrs_selftest.h"
#include "scene_internal.hpp"

using namespace rayrs;

// (never an empty buffer: a test of n == 0 values still passes its pointers to hipMemset)
static hipError_t alloc(DevBuf& b, size_t bytes) { return b.reserve(bytes ? bytes : 8); }

extern "C" {

int rayrs_test_math(int device, int fn, const double* x, const double* y, uint64_t n, double* out) {
    if (!x || !out) return RAYRS_INVALID_ARG;
    HIP_TRY(hipSetDevice(device));
    DevBuf dx, dy, dout;
    HIP_TRY(dx.upload(x, n * 8));
    if (y) HIP_TRY(dy.upload(y, n * 8));
    HIP_TRY(alloc(dout, n * 8));
    if (n) HIP_TRY(launch_test_math(fn, dx.as<const double>(), y ? dy.as<const double>() : nullptr, n, dout.as<double>(), nullptr));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(dout.download(out, n * 8));
    return RAYRS_OK;
}

int rayrs_test_rng(int device, uint64_t seed, const uint64_t* pixel, const uint64_t* sample, const uint32_t* draw,
                   uint64_t n, uint64_t* out_bits) {
    if (!pixel || !sample || !draw || !out_bits) return RAYRS_INVALID_ARG;
    HIP_TRY(hipSetDevice(device));
    DevBuf dp, ds, dd, dout;
    HIP_TRY(dp.upload(pixel, n * 8));
    HIP_TRY(ds.upload(sample, n * 8));
    HIP_TRY(dd.upload(draw, n * 4));
    HIP_TRY(alloc(dout, n * 8));
    if (n)
        HIP_TRY(launch_test_rng(seed, dp.as<const uint64_t>(), ds.as<const uint64_t>(), dd.as<const uint32_t>(), n,
                                dout.as<uint64_t>(), nullptr));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(dout.download(out_bits, n * 8));
    return RAYRS_OK;
}

int rayrs_test_intersect(rayrs_scene* scene, const double* o, const double* d, uint64_t n, int exact, double* t,
                         int64_t* object) {
    if (!scene || !o || !d || !t || !object) return RAYRS_INVALID_ARG;
    if (scene->device < 0) return RAYRS_NO_DEVICE;
    HIP_TRY(hipSetDevice(scene->device));
    DevBuf dorg, ddir, dt, dprim;
    HIP_TRY(dorg.upload(o, n * 24));
    HIP_TRY(ddir.upload(d, n * 24));
    HIP_TRY(alloc(dt, n * 8));
    HIP_TRY(alloc(dprim, n * 8));
    const SceneDev sc = make_scene_dev(scene, exact != 0);
    DevBuf dspill;  // stack entries beyond the LDS part, one strip per thread of the launch
    const uint64_t threads = (n + 255) / 256 * 256;
    if (sc.stack_depth > sc.stack_lds) HIP_TRY(alloc(dspill, stack_spill_words(sc, threads) * 4));
    if (n)
        HIP_TRY(launch_test_intersect(scene->flat.compact, sc, dorg.as<const double>(), ddir.as<const double>(), n,
                                      dt.as<double>(), dprim.as<long long>(), dspill.as<uint32_t>(), nullptr));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(dt.download(t, n * 8));
    HIP_TRY(dprim.download(object, n * 8));
    for (uint64_t i = 0; i < n; i++)  // DFS slot -> object index in insertion order
        if (object[i] >= 0) object[i] = (int64_t)scene->flat.prim_object[(size_t)object[i]];
    return RAYRS_OK;
}

int rayrs_test_trace(rayrs_scene* scene, const double* o, const double* d, uint64_t n, int exact, double* t, int64_t* object,
                     uint64_t* pre_answered) {
    if (!scene || !o || !d || !t || !object) return RAYRS_INVALID_ARG;
    if (scene->device < 0) return RAYRS_NO_DEVICE;
    HIP_TRY(hipSetDevice(scene->device));
    const bool ex = exact != 0;
    const SceneDev sc = make_scene_dev(scene, ex);
    // the pool: rayrs_tuning.pool_slots slots if set (the rays then go through it in chunks of that many), whole windows
    // (laid out as a render's, pool_wf: that includes the light entries, a quarter more memory, which no kernel run here touches)
    uint64_t np64 = scene->tuning.pool_slots ? scene->tuning.pool_slots : (n < (1u << 20) ? n : (1u << 20));
    const uint32_t np = (uint32_t)pool_whole_windows(np64 ? np64 : 1u);  // (at least one 1024)
    RenderDev rp;
    std::memset(&rp, 0, sizeof(rp));
    const TravPlan trav = trav_settings(scene, ex, np);
    trav.fill(rp);
    const uint32_t trav_blocks = trav.blocks;
    DevBuf dblock, dctl, dspill, dcount, dans, dorg, ddir;
    HIP_TRY(alloc(dblock, (size_t)np * POOL_SLOT_BYTES));
    HIP_TRY(alloc(dctl, sizeof(WfCtl)));
    HIP_TRY(alloc(dspill, stack_spill_words(sc, (uint64_t)trav_blocks * 256u) * 4u));
    HIP_TRY(alloc(dcount, sizeof(Counters)));
    HIP_TRY(alloc(dans, sizeof(unsigned long long)));
    HIP_TRY(alloc(dorg, (size_t)np * 24));
    HIP_TRY(alloc(ddir, (size_t)np * 24));
    HIP_TRY(hipMemset(dcount.as<>(), 0, sizeof(Counters)));
    HIP_TRY(hipMemset(dans.as<>(), 0, sizeof(unsigned long long)));
    const WfDev wf = pool_wf(dblock, np, dctl, trav_blocks, dspill);
    rp.counters = dcount.as<Counters>();
    std::vector<uint8_t> state(np);
    std::vector<PathSlot> slots(np);
    constexpr uint32_t MAX_ROUNDS = 64;
    for (uint64_t base = 0; base < n; base += np) {
        const uint32_t m = (uint32_t)(n - base < np ? n - base : np);
        HIP_TRY(hipMemcpy(dorg.as<>(), o + 3 * base, (size_t)m * 24, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(ddir.as<>(), d + 3 * base, (size_t)m * 24, hipMemcpyHostToDevice));
        HIP_TRY(wf_launch_intake(sc, wf, dorg.as<const double>(), ddir.as<const double>(), m, dans.as<unsigned long long>(), nullptr));
        // the traversal rounds of a render (render.cpp enqueue_streaming): there the hit kernel resets the window cursor
        uint32_t round = 0;
        for (;; round++) {
            WfCtl ctl;
            std::memset(&ctl, 0, sizeof(ctl));
            ctl.live_slots = m;
            HIP_TRY(hipMemcpy(dctl.as<>(), &ctl, sizeof(ctl), hipMemcpyHostToDevice));
            HIP_TRY(wf_launch_trav(scene->flat.compact, false, sc, rp, wf, trav_blocks, nullptr));
            HIP_TRY(hipDeviceSynchronize());
            HIP_TRY(hipMemcpy(state.data(), wf.state, np, hipMemcpyDeviceToHost));
            bool ready = false;
            for (uint32_t i = 0; i < m; i++) ready |= (state[i] & 7u) == WF_READY;
            if (!ready) break;
            if (round + 1 >= MAX_ROUNDS) {
                set_last_error("rayrs_test_trace: slots still READY after the traversal rounds");
                return RAYRS_HIP_ERROR;
            }
        }
        HIP_TRY(dblock.download(slots.data(), (size_t)m * sizeof(PathSlot)));  // (the block begins with the slot records)
        for (uint32_t i = 0; i < m; i++) {
            if (state[i] == WF_HIT) {
                if (slots[i].ray.prim >= scene->flat.prim_object.size()) {
                    set_last_error("rayrs_test_trace: a HIT slot names no primitive");
                    return RAYRS_HIP_ERROR;
                }
                t[base + i] = slots[i].ray.t;
                object[base + i] = (int64_t)scene->flat.prim_object[slots[i].ray.prim];  // DFS slot -> insertion order
            } else if (state[i] == WF_MISS) {
                t[base + i] = 0.0;
                object[base + i] = -1;
            } else {
                set_last_error("rayrs_test_trace: a slot left neither HIT nor MISS");
                return RAYRS_HIP_ERROR;
            }
        }
    }
    unsigned long long answered = 0;
    HIP_TRY(dans.download(&answered, sizeof(answered)));
    if (pre_answered) *pre_answered = answered;
    return RAYRS_OK;
}

int rayrs_test_path_trace(rayrs_scene* scene, const rayrs_camera* camera, uint64_t seed, uint32_t max_bounces,
                          const uint32_t* pixel, const uint32_t* sample, uint64_t n, int exact, uint32_t cap,
                          uint32_t* n_queries, int64_t* object, double* t, double* throughput, uint32_t* draw, double* rgb) {
    if (!scene || !camera || !pixel || !sample || !n_queries || !object || !t || !throughput || !draw || !rgb || cap == 0)
        return RAYRS_INVALID_ARG;
    if (scene->device < 0) return RAYRS_NO_DEVICE;
    for (uint64_t i = 0; i < n; i++)
        if ((pixel[i] >> 16) >= camera->y_pixels || (pixel[i] & 0xffffu) >= camera->x_pixels) return RAYRS_INVALID_ARG;
    HIP_TRY(hipSetDevice(scene->device));
    DevBuf dpix, dsam, dn, dprim, dt, dthr, ddraw, drgb, dspill;
    HIP_TRY(dpix.upload(pixel, n * 4));
    HIP_TRY(dsam.upload(sample, n * 4));
    HIP_TRY(alloc(dn, n * 4));
    HIP_TRY(alloc(dprim, n * cap * 4));
    HIP_TRY(alloc(dt, n * cap * 8));
    HIP_TRY(alloc(dthr, n * cap * 24));
    HIP_TRY(alloc(ddraw, n * cap * 4));
    HIP_TRY(alloc(drgb, n * 24));
    HIP_TRY(hipMemset(dprim.as<>(), 0xff, n * cap * 4));
    HIP_TRY(hipMemset(dt.as<>(), 0, n * cap * 8));
    HIP_TRY(hipMemset(dthr.as<>(), 0, n * cap * 24));
    HIP_TRY(hipMemset(ddraw.as<>(), 0, n * cap * 4));
    const SceneDev sc = make_scene_dev(scene, exact != 0);
    const CameraDev cam = make_camera_dev(camera);
    const uint64_t threads = (n + 255) / 256 * 256;
    if (sc.stack_depth > sc.stack_lds) HIP_TRY(alloc(dspill, stack_spill_words(sc, threads) * 4));
    if (n)
        HIP_TRY(launch_test_path_trace(scene->flat.compact, sc, cam, seed, max_bounces, dpix.as<const uint32_t>(),
                                       dsam.as<const uint32_t>(), n, cap, dn.as<uint32_t>(), dprim.as<uint32_t>(), dt.as<double>(),
                                       dthr.as<double>(), ddraw.as<uint32_t>(), drgb.as<double>(), dspill.as<uint32_t>(), nullptr));
    HIP_TRY(hipDeviceSynchronize());
    std::vector<uint32_t> prim(n * cap);
    HIP_TRY(dn.download(n_queries, n * 4));
    HIP_TRY(dprim.download(prim.data(), n * cap * 4));
    HIP_TRY(dt.download(t, n * cap * 8));
    HIP_TRY(dthr.download(throughput, n * cap * 24));
    HIP_TRY(ddraw.download(draw, n * cap * 4));
    HIP_TRY(drgb.download(rgb, n * 24));
    for (uint64_t k = 0; k < n * cap; k++)  // DFS slot -> object index in insertion order
        object[k] = prim[k] == 0xffffffffu ? -1 : (int64_t)scene->flat.prim_object[prim[k]];
    return RAYRS_OK;
}

int rayrs_test_material(int device, const rayrs_material* mat, const double* normal, const double* view,
                        const uint64_t* key, uint64_t n, int32_t* scattered, double* color, double* dir,
                        uint32_t* draws) {
    RAYRS_GUARDED({
    if (!mat || !normal || !view || !key || !scattered || !color || !dir || !draws) return RAYRS_INVALID_ARG;
    ObjectList tmp;
    const int surf = tmp.add_surface(mat, nullptr);
    if (surf < 0) return surf;
    HIP_TRY(hipSetDevice(device));
    DevBuf ds, dn, dv, dk, dsc, dc, dd, ddr;
    HIP_TRY(ds.upload(&tmp.surfaces[0], sizeof(SurfaceDev)));
    HIP_TRY(dn.upload(normal, n * 24));
    HIP_TRY(dv.upload(view, n * 24));
    HIP_TRY(dk.upload(key, n * 8));
    HIP_TRY(alloc(dsc, n * 4));
    HIP_TRY(alloc(dc, n * 24));
    HIP_TRY(alloc(dd, n * 24));
    HIP_TRY(alloc(ddr, n * 4));
    if (n)
        HIP_TRY(launch_test_material(ds.as<const SurfaceDev>(), dn.as<const double>(), dv.as<const double>(),
                                     dk.as<const uint64_t>(), n, dsc.as<int32_t>(), dc.as<double>(), dd.as<double>(),
                                     ddr.as<uint32_t>(), nullptr));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(dsc.download(scattered, n * 4));
    HIP_TRY(dc.download(color, n * 24));
    HIP_TRY(dd.download(dir, n * 24));
    HIP_TRY(ddr.download(draws, n * 4));
    return RAYRS_OK;
    })
}

int rayrs_test_background(rayrs_scene* scene, const double* dir, uint64_t n, double* rgb) {
    if (!scene || !dir || !rgb) return RAYRS_INVALID_ARG;
    if (scene->device < 0) return RAYRS_NO_DEVICE;
    HIP_TRY(hipSetDevice(scene->device));
    DevBuf dd, dout;
    HIP_TRY(dd.upload(dir, n * 24));
    HIP_TRY(alloc(dout, n * 24));
    const SceneDev sc = make_scene_dev(scene, false);
    if (n) HIP_TRY(launch_test_background(sc, dd.as<const double>(), n, dout.as<double>(), nullptr));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(dout.download(rgb, n * 24));
    return RAYRS_OK;
}

}  // extern "C"
