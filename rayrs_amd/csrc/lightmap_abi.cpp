// lightmap_abi.cpp -- the lightmap atlas of include/rayrs_hip.h (rayrs_lightmap_*): the refusals, the mesh widened and its
// triangles' normals made on the host (radiance_mesh_table.h mesh_tri_finish, the routine MESH LIGHTS' table uses), the three
// passes of lightmap.hip behind one another on the null stream, and an atlas's lifetime: after create it holds the owner plane
// and the texel list on its device, and what an assembly works in.
#include <hip/hip_runtime.h>

#include <memory>
#include <new>
#include <vector>

#include "../../include/rayrs_hip.h"
#include "device_mem.hpp"
#include "lightmap_kernels.h"
#include "radiance_mesh_table.h"
#include "rayrs_lab.h"
#include "scene_internal.hpp"

using namespace rayrs;

struct rayrs_lightmap {
    int device = -1;
    uint32_t w = 0, h = 0;
    uint64_t n = 0;
    DevBuf owner, index, points, normals, bary;  // the owner plane (h * w) and the texel list (n)
    DevBuf values, image[2], valid[2], changed;  // rayrs_lightmap_assemble: the rows, the two pairs of planes, a round's word
    double ms[3] = {0.0, 0.0, 0.0};              // create's owner pass, compaction and record pass (rayrs_lab_lightmap_ms)
};

// RAYRS_NO_DEVICE unless `device` is a HIP device of this machine.
static int device_check(int device) {
    int count = 0;
    if (device < 0 || hipGetDeviceCount(&count) != hipSuccess || device >= count) return RAYRS_NO_DEVICE;
    return RAYRS_OK;
}

extern "C" {

int rayrs_lightmap_create(int device, const void* verts, uint32_t vert_is_f32, uint32_t nv, const uint32_t* idx, uint32_t m,
                          const double* uvs, uint32_t width, uint32_t height, uint32_t flip, rayrs_lightmap** out) {
    RAYRS_GUARDED({
    if (!out) return RAYRS_INVALID_ARG;
    if (m > 0u && (!verts || !idx || !uvs)) return RAYRS_INVALID_ARG;
    if (vert_is_f32 > 1u || flip > 1u) return RAYRS_INVALID_ARG;
    if (width == 0u || height == 0u || width > RAYRS_LIGHTMAP_MAX_SIDE || height > RAYRS_LIGHTMAP_MAX_SIDE) return RAYRS_INVALID_ARG;
    for (size_t i = 0; i < (size_t)m * 3u; i++)
        if (idx[i] >= nv) return RAYRS_INVALID_ARG;
    RAYRS_TRY(device_check(device));
    HIP_TRY(hipSetDevice(device));

    // the vertices the triangles name, widened; a triangle's normal from its three
    std::vector<double> v((size_t)(m ? nv : 0u) * 3u), normals((size_t)m * 3u);
    for (size_t i = 0; i < v.size(); i++) v[i] = vert_is_f32 ? (double)static_cast<const float*>(verts)[i] : static_cast<const double*>(verts)[i];
    for (uint32_t k = 0; k < m; k++) {
        MeshTri t = {};
        for (int c = 0; c < 3; c++) {
            t.p1[c] = v[(size_t)idx[k * 3u] * 3u + c];
            t.p2[c] = v[(size_t)idx[k * 3u + 1u] * 3u + c];
            t.p3[c] = v[(size_t)idx[k * 3u + 2u] * 3u + c];
        }
        mesh_tri_finish(t);
        for (int c = 0; c < 3; c++) normals[(size_t)k * 3u + c] = flip ? -t.n[c] : t.n[c];
    }

    std::unique_ptr<rayrs_lightmap> lm(new rayrs_lightmap());
    lm->device = device, lm->w = width, lm->h = height;
    const uint64_t texels = (uint64_t)width * height;
    DevBuf d_verts, d_idx, d_uvs, d_normals, d_big, d_offsets, d_count;  // what only create needs
    HIP_TRY(d_verts.upload(v.data(), v.size() * sizeof(double)));
    HIP_TRY(d_idx.upload(idx, (size_t)m * 3u * sizeof(uint32_t)));
    HIP_TRY(d_uvs.upload(uvs, (size_t)m * 6u * sizeof(double)));
    HIP_TRY(d_normals.upload(normals.data(), normals.size() * sizeof(double)));
    HIP_TRY(d_big.reserve(((size_t)m + 1u) * sizeof(uint32_t)));
    HIP_TRY(d_offsets.reserve((size_t)lightmap_blocks(texels) * sizeof(uint32_t)));
    HIP_TRY(d_count.reserve(sizeof(LightmapCount)));
    HIP_TRY(lm->owner.reserve(texels * sizeof(uint32_t)));
    Event ev[4];
    for (Event& e : ev) HIP_TRY(e.create());

    LightmapDev dev;
    dev.verts = d_verts.as<double>(), dev.idx = d_idx.as<uint32_t>(), dev.uvs = d_uvs.as<double>(), dev.normals = d_normals.as<double>();
    dev.owner = lm->owner.as<uint32_t>(), dev.m = m, dev.w = width, dev.h = height;
    HIP_TRY(hipEventRecord(ev[0], nullptr));
    HIP_TRY(launch_lightmap_owner(dev, d_big.as<uint32_t>(), d_count.as<LightmapCount>(), nullptr));
    HIP_TRY(hipEventRecord(ev[1], nullptr));
    HIP_TRY(launch_lightmap_compact(dev, d_offsets.as<uint32_t>(), d_count.as<LightmapCount>(), nullptr));
    HIP_TRY(hipEventRecord(ev[2], nullptr));
    LightmapCount count = {};
    HIP_TRY(d_count.download(&count, sizeof(count)));  // (waits for the scan: the list's length sizes the list)
    lm->n = count.n;
    if (lm->n > 0u) {
        HIP_TRY(lm->index.reserve(lm->n * sizeof(uint32_t)));
        HIP_TRY(lm->points.reserve(lm->n * 3u * sizeof(double)));
        HIP_TRY(lm->normals.reserve(lm->n * 3u * sizeof(double)));
        HIP_TRY(lm->bary.reserve(lm->n * 3u * sizeof(double)));
        const LightmapList list{lm->index.as<uint32_t>(), lm->points.as<double>(), lm->normals.as<double>(), lm->bary.as<double>()};
        HIP_TRY(launch_lightmap_records(dev, d_offsets.as<uint32_t>(), list, nullptr));
    }
    HIP_TRY(hipEventRecord(ev[3], nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    for (int k = 0; k < 3; k++) {
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, ev[k], ev[k + 1]));
        lm->ms[k] = (double)t;
    }
    *out = lm.release();
    return RAYRS_OK;
    })
}

void rayrs_lightmap_destroy(rayrs_lightmap* lm) {
    if (!lm) return;
    if (lm->device >= 0) (void)hipSetDevice(lm->device);
    delete lm;
}

int rayrs_lightmap_count(const rayrs_lightmap* lm, uint64_t* n) {
    if (!lm || !n) return RAYRS_INVALID_ARG;
    *n = lm->n;
    return RAYRS_OK;
}

int rayrs_lightmap_texels(rayrs_lightmap* lm, uint32_t* index, double* points, double* normals, double* bary) {
    RAYRS_GUARDED({
    if (!lm) return RAYRS_INVALID_ARG;
    if (lm->n == 0u) return RAYRS_OK;
    HIP_TRY(hipSetDevice(lm->device));
    if (index) HIP_TRY(lm->index.download(index, lm->n * sizeof(uint32_t)));
    if (points) HIP_TRY(lm->points.download(points, lm->n * 3u * sizeof(double)));
    if (normals) HIP_TRY(lm->normals.download(normals, lm->n * 3u * sizeof(double)));
    if (bary) HIP_TRY(lm->bary.download(bary, lm->n * 3u * sizeof(double)));
    return RAYRS_OK;
    })
}

int rayrs_lightmap_owner(rayrs_lightmap* lm, uint32_t* owner) {
    RAYRS_GUARDED({
    if (!lm || !owner) return RAYRS_INVALID_ARG;
    HIP_TRY(hipSetDevice(lm->device));
    HIP_TRY(lm->owner.download(owner, (size_t)lm->w * lm->h * sizeof(uint32_t)));
    return RAYRS_OK;
    })
}

int rayrs_lightmap_assemble(rayrs_lightmap* lm, const double* values, uint32_t channels, int32_t dilate, double* image, uint8_t* valid) {
    RAYRS_GUARDED({
    if (!lm) return RAYRS_INVALID_ARG;
    if ((lm->n > 0u && !values) || !image) return RAYRS_INVALID_ARG;
    if (channels < 1u || channels > 4u || dilate < 0) return RAYRS_INVALID_ARG;
    HIP_TRY(hipSetDevice(lm->device));
    const uint64_t texels = (uint64_t)lm->w * lm->h;
    const size_t image_bytes = (size_t)texels * channels * sizeof(double);
    HIP_TRY(lm->image[0].reserve(image_bytes));
    HIP_TRY(lm->valid[0].reserve(texels));
    HIP_TRY(lm->changed.reserve(sizeof(uint32_t)));
    if (lm->n > 0u) HIP_TRY(lm->values.upload(values, (size_t)lm->n * channels * sizeof(double)));
    HIP_TRY(launch_lightmap_scatter(lm->index.as<uint32_t>(), lm->n, lm->values.as<double>(), channels, texels, lm->image[0].as<double>(),
                                    lm->valid[0].as<uint8_t>(), nullptr));
    int cur = 0;
    for (int32_t round = 0; round < dilate; round++) {
        HIP_TRY(lm->image[cur ^ 1].reserve(image_bytes));
        HIP_TRY(lm->valid[cur ^ 1].reserve(texels));
        HIP_TRY(hipMemsetAsync(lm->changed.as<>(), 0, sizeof(uint32_t), nullptr));
        HIP_TRY(launch_lightmap_dilate(lm->image[cur].as<double>(), lm->valid[cur].as<uint8_t>(), lm->image[cur ^ 1].as<double>(),
                                       lm->valid[cur ^ 1].as<uint8_t>(), lm->w, lm->h, channels, lm->changed.as<uint32_t>(), nullptr));
        uint32_t changed = 0u;
        HIP_TRY(lm->changed.download(&changed, sizeof(changed)));
        if (!changed) break;  // (the round wrote a copy of its input: every later one would)
        cur ^= 1;
    }
    HIP_TRY(lm->image[cur].download(image, image_bytes));
    if (valid) HIP_TRY(lm->valid[cur].download(valid, texels));
    return RAYRS_OK;
    })
}

int rayrs_lab_lightmap_ms(const rayrs_lightmap* lm, double ms[3]) {
    if (!lm || !ms) return RAYRS_INVALID_ARG;
    for (int k = 0; k < 3; k++) ms[k] = lm->ms[k];
    return RAYRS_OK;
}

}  // extern "C"
