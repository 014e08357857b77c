// radiance_lit_host.hpp -- what the four units of entry points that take a light list share (radiance_lit_abi.cpp: LIGHT SAMPLING,
// radiance_direct_abi.cpp: DIRECT LIGHTING, radiance_sky_abi.cpp: SKY SAMPLING, radiance_mesh_abi.cpp: MESH LIGHTS): a call's
// description and its way from the refusals through the launches, all in radiance_lit_abi.cpp.  A call differs between them in
// `direct`, `sky` and `mesh` alone.
#pragma once
#include <memory>
#include <vector>

#include "../../include/rayrs_hip.h"
#include "device_mem.hpp"
#include "radiance_direct_kernels.h"
#include "radiance_lit_kernels.h"
#include "radiance_mesh_table.h"
#include "radiance_sky_table.h"
#include "radiance_tree_table.h"
#include "scene_internal.hpp"

// A mesh-light group (include/rayrs_hip.h MESH LIGHTS): bound to its scene, it owns the host table (radiance_mesh_table.h: P,
// the records; the bitmap over the scene's primitive slots) and the device copy, uploaded at the first call that launches.
struct rayrs_mesh_lights {
    rayrs_scene* scene = nullptr;
    uint32_t n = 0;
    double total = 0.0;
    std::vector<double> table;     // mesh_table_bytes(n) / 8 doubles; empty with n == 0
    std::vector<uint32_t> listed;
    bool uploaded = false;
    rayrs::DevBuf d_table, d_listed;
    // LIGHT TREE (rayrs_mesh_lights_create_tree, radiance_tree_abi.cpp): the selection is the tree.  The records of `table` carry
    // path, depth and w; `nodes` and `entry` are radiance_tree_table.h's, `listed` stays empty; pre_* are the nodes in the
    // header's preorder numbering (2N - 1 of them), for rayrs_mesh_lights_tree_nodes.
    bool tree = false;
    std::vector<rayrs::TreeNode> nodes;
    std::vector<uint32_t> entry;
    std::vector<double> pre_mrw;               // m, r2, W: five per node
    std::vector<uint32_t> pre_right, pre_entry;  // the right child's index / the leaf's entry, 0xFFFFFFFF where there is none
    rayrs::DevBuf d_nodes, d_entry;
    ~rayrs_mesh_lights();  // waits for the scene's radiance work, which may still read the device copy (radiance_mesh_abi.cpp)
};

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
    // MESH LIGHTS (with direct): a handle of another scene is refused; one of N >= 1 triangles takes radiance_mesh.hip's kernels,
    // a tree handle (LIGHT TREE) of N >= 1 radiance_tree.hip's
    const rayrs_mesh_lights* mesh = nullptr;
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

// The depth-first slot of every object (the inverse of flat.prim_object, made once), and the tag of the primitive in a slot and
// its record (layout.h).
const std::vector<uint32_t>& lit_object_prim(rayrs_scene* scene);
const uint32_t* prim_record(const rayrs_scene* scene, uint32_t p);
uint32_t lit_prim_tag(const rayrs_scene* scene, uint32_t p);

// The group as the kernels take it, with the device copy, uploaded at the handle's first call (the scene's device is current;
// mesh->n >= 1) (radiance_mesh_abi.cpp).
int mesh_device_table(const rayrs_mesh_lights* mesh, MeshDev* out);
// rayrs_mesh_lights_create past its null checks: the list's refusals in the header's order, then the handle with its table
// (radiance_mesh_abi.cpp).
int mesh_lights_make(rayrs_scene* scene, const uint32_t* tris, uint64_t n_tris, std::unique_ptr<rayrs_mesh_lights>& m);

// A tree handle's group as the kernels take it, with the device copy, uploaded at the handle's first call (the scene's device is
// current; mesh->tree, mesh->n >= 1), and rayrs_mesh_lights_density on a tree handle past its refusals (radiance_tree_abi.cpp).
int tree_device_table(const rayrs_mesh_lights* mesh, TreeDev* out);
int tree_host_density(const rayrs_mesh_lights* mesh, const double* position, const uint32_t* j, const double* q, uint64_t n, double* p);

// The sky's table of the host scene's HDRI, built at the first call (radiance_sky_abi.cpp); `table` is a host pointer.
SkyDev sky_host_table(rayrs_scene* scene);
// T > 0.0 and finite: there is something to sample.
bool sky_table_usable(rayrs_scene* scene);
// The same with the device copy, uploaded at the first call (the scene's device is current).
int sky_device_table(rayrs_scene* scene, SkyDev* out);

}  // namespace rayrs
