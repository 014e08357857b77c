/*
 * rayrs_hip.h -- C ABI of the MI355X (gfx950) build of rayrs-lib's per-pixel
 * radiance integrator.
 *
 * The reference (Frojdholm/rayrs) has no FFI: its finest seam is the Rust
 * call pair Camera::generate_primary_ray (rayrs-lib/src/lib.rs:202) +
 * rayrs_lib::radiance (lib.rs:521) inside the rayon block loop of
 * rayrs/src/main.rs:57-101.  A per-ray FFI is useless for a GPU, so this
 * boundary is per image: rayrs_render replaces main.rs:57-101 wholesale, and
 * because Scene/Object/Camera keep their fields private (lib.rs:56-67,
 * :216-220, :302-306) the constructors are part of the boundary too.  Each
 * entry point names the reference item it stands for; INTEGRATION.md shows
 * the Rust `extern "C"` block a maintainer would add to rayrs-lib.
 *
 * Conventions: every function returns 0 (RAYRS_OK) or a negative
 * rayrs_status; nothing unwinds or aborts across the boundary.  Parameter
 * checks are the reference's assert!s turned into RAYRS_INVALID_ARG.  Plain
 * pointers and sizes only; device pointers are passed as void*.
 */
#ifndef RAYRS_HIP_H
#define RAYRS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    RAYRS_OK = 0,
    RAYRS_INVALID_ARG = -1, /* a reference assert! would have fired */
    RAYRS_HIP_ERROR = -2,   /* a HIP runtime call failed (see rayrs_last_error) */
    RAYRS_OOM = -3,
    RAYRS_NO_DEVICE = -4,   /* scene was created host-only or no GPU present */
    RAYRS_UNSUPPORTED = -5, /* more than 2^32 (pixel, sample chunk) items on a rank; max_bounces > 8000 (8000 itself is
                               accepted: bounce count and draw index travel as 16 bits, a bounce draws at most four
                               numbers); an image side > 65535; a walk tree that needs more than 4096 stack entries */
    RAYRS_IO_ERROR = -6,    /* file missing or malformed (see rayrs_io_last_error) */
    RAYRS_RCCL_ERROR = -7   /* the RCCL library could not be loaded, or one of its calls failed (rayrs_render_multi) */
} rayrs_status;

const char* rayrs_strerror(int status);
/* Text of the last HIP error seen by the calling thread ("" if none). */
const char* rayrs_last_error(void);

/* ---- material.rs ---- */

/* enum Material, material.rs:57-68 */
enum {
    RAYRS_MAT_LAMBERTIAN = 0,            /* LambertianDiffuse::new(color)              :608 */
    RAYRS_MAT_REFLECT = 1,               /* Reflect::new(color)                        :629 */
    RAYRS_MAT_REFRACT = 2,               /* Refract::new(color, ior)                   :650 */
    RAYRS_MAT_GLASS = 3,                 /* Glass::new(color, ior)                     :673 */
    RAYRS_MAT_COOK_TORRANCE = 4,         /* CookTorrance::new(color, alpha, fresnel)   :705 */
    RAYRS_MAT_COOK_TORRANCE_REFRACT = 5, /* CookTorranceRefract::new(color, alpha, ior):832 */
    RAYRS_MAT_COOK_TORRANCE_GLASS = 6,   /* CookTorranceGlass::new(color, alpha, ior)  :863 */
    RAYRS_MAT_PLASTIC = 7,               /* Plastic::new(color, spec_color, alpha, ior):887 */
    RAYRS_MAT_NO_REFLECT = 8             /* Material::NoReflect                            */
};

typedef struct {
    int32_t kind;         /* RAYRS_MAT_* */
    int32_t metallic;     /* CookTorrance: 1 = Fresnel::SchlickMetallic(r0), 0 = SchlickDielectric(ior) (:128-131) */
    double color[3];
    double spec_color[3]; /* Plastic only */
    double alpha;         /* roughness; stored squared like the reference ctor (:711) */
    double ior;
    double r0[3];
} rayrs_material;

/* enum Emission, material.rs:1056-1075; emissive = 0 is Emission::Dark */
typedef struct {
    int32_t emissive;
    int32_t pad;
    double strength;
    double color[3];
} rayrs_emission;

/* enum Axis, geometry.rs:161-168 */
enum { RAYRS_AXIS_X = 0, RAYRS_AXIS_XREV = 1, RAYRS_AXIS_Y = 2, RAYRS_AXIS_YREV = 3, RAYRS_AXIS_Z = 4, RAYRS_AXIS_ZREV = 5 };

/* enum BvhHeuristic, bvh.rs:187-191 */
enum { RAYRS_BVH_MIDPOINT = 0, RAYRS_BVH_SAH = 1 };

/* ---- Vec<Object>: lib.rs:302-512 ---- */

typedef struct rayrs_objects rayrs_objects;

int rayrs_objects_create(rayrs_objects** out);
void rayrs_objects_destroy(rayrs_objects* objs);
uint64_t rayrs_objects_len(const rayrs_objects* objs);

/* Object::sphere(radius, origin, mat, emission)                     lib.rs:321 */
int rayrs_object_sphere(rayrs_objects* objs, double radius, const double origin[3], const rayrs_material* mat,
                        const rayrs_emission* emission);
/* Object::plane(axis, umin, umax, vmin, vmax, pos, mat, emission)   lib.rs:342 */
int rayrs_object_plane(rayrs_objects* objs, int axis, double umin, double umax, double vmin, double vmax, double pos,
                       const rayrs_material* mat, const rayrs_emission* emission);
/* Object::triangle(p1, p2, p3, mat, emission)                       lib.rs:380 */
int rayrs_object_triangle(rayrs_objects* objs, const double p1[3], const double p2[3], const double p3[3],
                          const rayrs_material* mat, const rayrs_emission* emission);
/* Object::from_triangles(tris, mat, emission)                       lib.rs:407
 * as an indexed mesh: verts = nverts*3 coordinates, idx = ntris*3 vertex
 * indices (0-based, counter-clockwise).  The f32 form is what a PLY file
 * holds; the values are widened to f64 exactly. */
int rayrs_object_from_triangles_f32(rayrs_objects* objs, const float* verts, uint32_t nverts, const uint32_t* idx,
                                    uint32_t ntris, const rayrs_material* mat, const rayrs_emission* emission);
int rayrs_object_from_triangles_f64(rayrs_objects* objs, const double* verts, uint32_t nverts, const uint32_t* idx,
                                    uint32_t ntris, const rayrs_material* mat, const rayrs_emission* emission);
/* Object::from_spheres(spheres, mat, emission)                      lib.rs:422
 * centers = n*3 */
int rayrs_object_from_spheres(rayrs_objects* objs, double radius, const double* centers, uint32_t n,
                              const rayrs_material* mat, const rayrs_emission* emission);
/* Object::box_geom(lower_left, upper_right, mat, emission)          lib.rs:438 */
int rayrs_object_box_geom(rayrs_objects* objs, const double lower_left[3], const double upper_right[3],
                          const rayrs_material* mat, const rayrs_emission* emission);

/* ---- Scene: lib.rs:216-296 ---- */

typedef struct rayrs_scene rayrs_scene;

/* Scene::new(objects, z_near, z_far, heuristic, hdri)               lib.rs:227
 * Consumes nothing: `objs` stays owned by the caller and may be destroyed
 * right after.  Builds the BVH exactly as Bvh::build does (bvh.rs:199-389,
 * same splits, same child order), derives the tree the kernels walk from it
 * (rayrs_scene_export_wide) and uploads that to HIP device `device`.  device = -1 builds a host-only scene (no GPU needed) that can
 * be inspected with rayrs_scene_info / rayrs_scene_export_bvh but not
 * rendered.  hdri_rgb: hdri_w*hdri_h RGB f32 texels, row-major, image origin
 * upper left; values are clipped to [0, 3] as main.rs:43 does. */
int rayrs_scene_new(const rayrs_objects* objs, double z_near, double z_far, int heuristic, uint32_t splits,
                    uint32_t hdri_w, uint32_t hdri_h, const float* hdri_rgb, int device, rayrs_scene** out);
void rayrs_scene_destroy(rayrs_scene* scene);

typedef struct {
    uint64_t n_objects;
    uint32_t n_interior;   /* two-child records */
    uint32_t n_prims;      /* leaf primitives in DFS order (== n_objects) */
    uint32_t root_ref;
    uint32_t depth;        /* levels of interior records */
    uint32_t compact;      /* 1 = f32 node boxes / f32 triangle vertices (exactly representable) */
    uint32_t n_surfaces;
    uint32_t node_bytes;   /* bytes of one wide interior record on the device */
    uint32_t prim_bytes;   /* bytes of one primitive record on the device */
    uint64_t device_bytes; /* total scene footprint in HBM */
    double root_box[6];    /* xmin,xmax,ymin,ymax,zmin,zmax */
    double build_seconds;
    uint32_t n_wide;        /* four-slot records of the tree the fast walk reads (rayrs_scene_export_wide) */
    uint32_t wide_root_ref;
    uint32_t wide_depth;    /* stack entries the traversal can need */
    uint32_t local_pool;    /* 1 = the gate tree is at most one record: renders keep every path in LDS
                               (rayrs_tuning.local_pool, local_pool.hip) */
    uint32_t gate_n_wide;   /* the same three for the gate tree (rayrs_scene_export_gate_tree), which */
    uint32_t gate_root_ref; /* the default walk reads */
    uint32_t gate_depth;
    /* The default walk's HOT GROUP (hot_count = 0: the scene has none): one group of the gate tree -- the one whose
     * gating box is the largest, if it covers at least a quarter of the root Node's box: on the reference's obj scenes the
     * floor's bottom Node, which nine rays in ten enter -- is left out of the records the default walk reads
     * (rayrs_scene_export_hot_tree: hot_n_wide records) and tested ONCE PER RAY outside that tree, by the kernel that
     * makes the ray, for a whole batch of rays together: its gating box hot_box exactly as
     * AxisAlignedBoundingBox::intersect tests it, then its hot_count primitives hot_first ... in depth-first order
     * exactly as the reference tests them -- on wave-uniform f64 values.  The groups of that tree and
     * the hot group together are the groups of the gate tree, each behind its gating box: the primitives tested are
     * still exactly those BvhTree::intersect tests (tests/test_bvh_builder.py checks it from the exports). */
    uint32_t hot_n_wide;
    uint32_t hot_root_ref;
    uint32_t hot_depth;
    uint32_t hot_first;
    uint32_t hot_count;
    uint32_t hot_pad;
    double hot_box[6];
} rayrs_scene_info_t;

int rayrs_scene_info(const rayrs_scene* scene, rayrs_scene_info_t* info);
/* The same scene (BVH, records, materials, HDRI, tuning) uploaded to another HIP device without
 * building it again: what rayrs_render_multi wants one of per GPU.  `scene` may be host-only. */
int rayrs_scene_clone_to_device(const rayrs_scene* scene, int device, rayrs_scene** out);
/* HIP device of the scene, -1 for a host-only scene. */
int rayrs_scene_device(const rayrs_scene* scene);
/* child_box: n_interior*2*6 f64, child_ref: n_interior*2 u32, prim_object:
 * n_prims u32 (index of the object, in insertion order, at each DFS slot).
 * ref = kind<<30 | payload; kind 0 = interior record (payload = index),
 * 1 = 1..4 primitives behind a box test (payload = first<<2 | count-1),
 * 2 = one primitive with no box test (payload = prim<<2). */
int rayrs_scene_export_bvh(const rayrs_scene* scene, double* child_box, uint32_t* child_ref, uint32_t* prim_object);
/* The records the kernels walk (wide_box: n*4*6 f64, wide_ref: n*4 u32, kind 3 = unused slot): NOT the
 * reference's topology but trees built for traversal speed.  What decides whether BvhTree::intersect reaches a
 * primitive is one box, its GATING box -- the box of the Node it hangs under; boxes on a root path nest exactly and
 * the slab test is monotone in the bounds, so passing it implies passing every box above.
 *   rayrs_scene_export_gate_tree (n = gate_n_wide): a leaf slot (kind 1) is one of the reference's groups -- the
 * 1..4 leaves that share a parent Node, contiguous in depth-first order -- behind exactly its gating box; an
 * interior slot (kind 0) carries the union of the boxes below it, so a ray that misses it misses every gating box
 * inside.  Every group appears exactly once: the primitives this tree reaches are the primitives the reference
 * reaches.  Walked by default, and the source of the local-pool route's gates.
 *   rayrs_scene_export_wide (n = n_wide), what rayrs_render_params.fast_traversal walks: a leaf slot is ONE primitive behind its own bounding box
 * (Bvh::build's, geometry.rs bbox) widened on every side by 1/64 of its largest extent, rounded outwards to f32 and
 * clipped to its gating box.  It reaches a subset of what the reference reaches (see fast_traversal for what the
 * subset leaves out: a bet).
 * tests/test_bvh_builder.py checks all of this from the exports alone. */
int rayrs_scene_export_wide(const rayrs_scene* scene, double* wide_box, uint32_t* wide_ref);
int rayrs_scene_export_gate_tree(const rayrs_scene* scene, double* wide_box, uint32_t* wide_ref);
/* The gate tree without the hot group (rayrs_scene_info_t.hot_*; n = hot_n_wide): what the default walk reads on a scene
 * that has one.  RAYRS_INVALID_ARG on a scene without a hot group. */
int rayrs_scene_export_hot_tree(const rayrs_scene* scene, double* wide_box, uint32_t* wide_ref);

/* ---- Camera: lib.rs:54-211 ---- */

typedef struct {
    double origin[3];
    double e_x[3];
    double e_y[3];
    double z[3];
    double width, height;
    uint32_t ppc;
    uint32_t x_pixels; /* Camera::x_pixels lib.rs:153 */
    uint32_t y_pixels; /* Camera::y_pixels lib.rs:175 */
} rayrs_camera;

/* Camera::new(origin, up, lookat, fov, width, height, ppi)          lib.rs:99 */
int rayrs_camera_new(const double origin[3], const double up[3], const double lookat[3], double fov, double width,
                     double height, uint32_t ppi, rayrs_camera* out);

/* ---- render: the block loop of rayrs/src/main.rs:57-101 ---- */

enum { RAYRS_OUT_F32 = 0, RAYRS_OUT_F64 = 1 };

typedef struct {
    uint32_t spp;          /* main.rs:68 */
    uint32_t max_bounces;  /* main.rs:77 passes 50 */
    uint64_t seed;         /* build-defined RNG, include/rayrs_numeric.h */
    /* Pixels are summed per pixel in chunks of `sample_chunk` consecutive
     * samples; chunk sums are added in chunk order.  0 or >= spp reproduces
     * the reference's single sequential sum (main.rs:67-79). */
    uint32_t sample_chunk;
    /* Image tiles (8x8 pixels, row-major tile index t) with
     * t % tile_ranks == tile_rank are rendered; other pixels of `out` are not
     * written.  1-GPU: tile_rank 0, tile_ranks 1. */
    uint32_t tile_rank, tile_ranks;
    uint32_t out_format;   /* RAYRS_OUT_F32: f32x3 (image.rs:224-229), RAYRS_OUT_F64: f64x3 */
    uint32_t count_work;   /* 1 = also count traversal work (slower; for the roofline figure) */
    /* Which walk answers the BVH queries.  BvhTree::intersect tests every primitive whose enclosing Node boxes the
     * ray enters and never compares a box with the closest hit so far (bvh.rs:391-415).
     * 0 (default): the walk over the reference's leaf groups behind their exact gating boxes
     *   (rayrs_scene_export_gate_tree) with nothing culled: it tests exactly the primitives the reference tests, so
     *   its closest hit (smallest accepted t, first primitive in depth-first order on ties, bvh.rs:62) is the
     *   reference's for EVERY ray BY CONSTRUCTION.  The local-pool route walks this way too.  Which kernel makes a
     *   test, and when, is the library's business: on a scene with a hot group (rayrs_scene_info_t.hot_count) the root
     *   box, that group and the first record of the tree without it are tested by the kernel that makes the ray, the
     *   rest by the traversal kernel -- the same tests on the same values, the same set of primitives.
     * 1: the fast walk, which makes two bets on the reference's arithmetic, each measured, neither a construction
     *   (it was the default until round 5; the headline frame renders 10 % faster with it -- 23 % before round 6 moved
     *   the default walk's cheap tests out of the traversal kernel, profiles/r05_walks.txt, r06_final_bench.json):
     *   - closest-hit culling: a box entered beyond best_t * (1 + 2^-10) is skipped -- the reference's answer
     *     unless a primitive's COMPUTED t lies more than that in front of a box around it;
     *   - tight leaf boxes (rayrs_scene_export_wide): a primitive is tested only if the ray enters its own bounding
     *     box widened by 1/64 of its size (inside the reference's gating box, so nothing extra is ever tested) --
     *     the reference's answer unless its own test accepts a hit on a primitive the ray passes beside by more
     *     than that.
     *   Both fail only for rays aimed nearly IN a primitive's plane, where Moeller-Trumbore's own result is rounding
     *   noise, and the failure envelope below is MEASURED, not proven (scripts/fuzz_traversal.py, 4 * 10^7 rays on sliver
     *   meshes and nearly flat sheets, profiles/r05_fuzz_traversal.txt; "near" = from within the camera rule below):
     *   - in-plane rays at 1e-7 rad and MORE off the plane, from nearby: 17 wrong hits in 3.97 M such rays, all on finely
     *     tessellated sheets of SLIVER quads (250-400 per side, aspect ratios up to 10^6: the culling bet fails there at
     *     any distance; 1 of the 17 is lost by the leaf boxes alone); none on the coarser sheets;
     *   - closer than 1e-7 rad to the plane, from nearby: 52 in 5.96 M (31 of them by the leaf boxes alone);
     *   - from far away (beyond the camera rule) the leaf boxes fail for about one in-plane ray in 10^4 at 1e-9 rad and
     *     more, seven in 10^4 closer to the plane.
     *   tests/test_walk_tree.py pins one failing ray of each kind, on which the default walk returns the reference's
     *   primitive.  No rendered frame, of any size, has differed in a bit -- pixels are not aimed along triangle planes.
     *   The camera rule: a frame whose camera stands farther from the scene's bounding box than 8 times that box's
     *   diagonal, or than 4096 times the scene's small-primitive extent (the 5th percentile of the primitives' largest
     *   extents), takes the default walk whatever it asked for (rayrs_render_stats.exact_walk reports the walk a frame
     *   took).  The rule looks at the camera, so it guards PRIMARY rays only: a bounced ray that travels from a large
     *   surface to a finely tessellated one covers thousands of small-primitive sizes and makes the leaf-box bet in the
     *   regime where it was seen to fail; and on a finely tessellated scene most real cameras count as far, so the field
     *   is then ignored (visible only in exact_walk).
     * What a sound walk costs, and what certificates (a forward error bound of Moeller-Trumbore deciding where "box
     * missed" provably means "rejected") could and could not buy back: profiles/r05_certified_walks.txt, DESIGN.md 2.
     * Zero-initialise the struct: values above 1 are refused (RAYRS_INVALID_ARG).  (Until round 5 this field was
     * `exact_traversal` with the opposite sense.) */
    uint32_t fast_traversal;
} rayrs_render_params;

typedef struct {
    uint64_t rays;          /* BVH queries = radiance loop iterations, lib.rs:525-526 */
    uint64_t paths;
    uint64_t nan_pixels;    /* main.rs:81-83 */
    uint64_t neg_pixels;    /* main.rs:85-87 */
    uint64_t interior_visits; /* the next five only with count_work */
    uint64_t tri_tests;
    uint64_t sphere_tests;
    uint64_t plane_tests;
    uint64_t escaped_paths;
    /* lane-utilisation diagnostics (count_work only); each *_wave value is summed over
     * all 64 lanes of the waves that executed the phase, *_lane over the active lanes */
    uint64_t step_wave, step_lane, inner_wave, leaf_wave;
    /* shader-clock ticks the traversal kernel's waves spent in interior steps, in leaf steps
     * and in retiring/refilling (count_work only), summed over waves */
    uint64_t interior_ticks, leaf_ticks;
    double kernel_ms;       /* summed HIP-event time of the traversal kernel's launches on its stream (the local-pool
                               kernel's when local_pool is set) */
    double total_ms;        /* all kernels of the render: path rounds + resolve */
    uint64_t kernel_launches; /* launches of the traversal kernel (= path rounds) */
    double trace_ms;        /* all path rounds (gen + traversal + hit + miss kernels) */
    uint64_t refill_ticks;
    /* closest hits by surface (count_work only): surface_hits[k] = BVH queries whose closest hit carries
     * the k-th distinct (Material, Emission) pair in object insertion order, pairs 7 and up together;
     * rays - sum(surface_hits) = queries that found nothing (Scene::background) */
    uint64_t surface_hits[8];
    /* primary rays that missed the root Node's box (bvh.rs:394: a Miss before anything else is looked at): their
     * samples are finished by the kernel that made the ray, without a trip through the traversal and miss
     * kernels.  They are part of `rays` and of `escaped_paths`. */
    uint64_t direct_rays;
    double hit_ms, miss_ms; /* summed HIP-event times of the hit and the miss kernel's launches (kernel_ms: the traversal
                               kernel's, or the local-pool kernel's, which is then the only one) */
    uint32_t local_pool;    /* 1 = this frame was rendered by the local-pool kernel (rayrs_tuning.local_pool) */
    uint32_t exact_walk;    /* 1 = this frame's queries were answered by the reference's visit set (the default); 0 = by the
                               fast walk (rayrs_render_params.fast_traversal = 1, the camera near enough, the streaming
                               route: the local-pool route never makes the bets) */
    uint32_t hot_group;     /* 1 = ... with the scene's hot group (rayrs_scene_info_t.hot_count) and the first record of the walk tree
                               tested by the kernels that MAKE the rays, for whole batches at once: a ray whose query ends
                               there never travels through the traversal kernel */
    uint32_t stats_pad;
    uint64_t pre_rays;        /* the next five only with count_work: queries (of `rays`) that were answered by the kernel that made
                                 the ray -- bounced rays that miss the root box, rays that enter no slot of the walk tree's first record */
    uint64_t pre_root_records;/* ... of them, the rays that entered the root box: each is one visit of the walk tree's first record
                                 (counted in interior_visits) that ended the query */
    uint64_t hot_lane;        /* rays put to the hot group's gating box */
    uint64_t hot_prim_tests;  /* of tri_tests + sphere_tests + plane_tests, the hot group's */
    uint64_t hot_tri_divided; /* ... of its triangle tests, those that went on to the three divisions (the others were settled
                                 before them by two exact facts about IEEE division: device_path.h hot_triangle_intersect) */
} rayrs_render_stats;

/* The sample chunk a frame is rendered with when the caller has no reason to choose another:
 * the smallest `requested` * 2^k (requested = 0 means 4) for which the WHOLE frame -- all of its
 * 8x8 tiles, whoever renders them -- has at most 2^30 (pixel, chunk) items.  It depends on the
 * frame only, never on the number of GPUs that share it, so that every rank count sums a pixel's
 * samples in the same order and produces the same bits.  (Each rank keeps 24 bytes of partial
 * sum per item; a rank refuses more than 2^32 items.) */
uint32_t rayrs_frame_sample_chunk(uint32_t x_pixels, uint32_t y_pixels, uint32_t spp, uint32_t requested);

/* Renders into a HOST buffer of y_pixels*x_pixels*3 elements (row-major,
 * origin upper left, RGB).  Synchronous. */
int rayrs_render(rayrs_scene* scene, const rayrs_camera* camera, const rayrs_render_params* params, void* out_host,
                 rayrs_render_stats* stats);

/* Enqueues the render on `hip_stream` (a hipStream_t, NULL = default stream) writing a DEVICE
 * buffer of the same shape.  The number of path rounds is data dependent (a frame ends when the
 * last path does), so rounds are enqueued in batches and the call reads the live-path count of
 * batch b back while batch b+1 is already queued: it returns once the LAST batch is enqueued --
 * the GPU is never idle waiting for the host, but the call itself lasts about as long as the
 * frame minus its last batch.  The resolve pass and everything the caller enqueues on the stream
 * afterwards (an RCCL reduce, a copy) is ordered behind the render without a host wait. */
int rayrs_render_launch(rayrs_scene* scene, const rayrs_camera* camera, const rayrs_render_params* params,
                        void* out_device, void* hip_stream);
/* Waits for the last rayrs_render_launch on this scene and returns its counters. */
int rayrs_render_finish(rayrs_scene* scene, rayrs_render_stats* stats);

/* The same block loop over several GPUs of one node, inside the library (the reference does all of
 * its parallelism -- rayon over image blocks, main.rs:57-101 -- inside the product too).  scenes[i]
 * are n handles of the same scene on the devices to use (rayrs_scene_clone_to_device); rank i renders
 * the 8x8 tiles t with t % n == i from its own host thread on its own stream into a zeroed
 * framebuffer on its device, and one RCCL reduce (sum, over xGMI) to scenes[0]'s device assembles
 * the frame, which is copied to out_host.  A pixel is non-zero on exactly one rank, so the frame
 * equals the one-GPU frame bit for bit.  params->tile_rank / tile_ranks are ignored.  Handles on the
 * same device are allowed (rehearsal on one GPU): their buffers are summed on that device first.
 * RCCL is loaded at the first call that spans more than one device; RAYRS_RCCL_ERROR if that or a collective
 * fails.  stats: every counter summed over the ranks; times and kernel_launches = the slowest rank's. */
int rayrs_render_multi(rayrs_scene* const* scenes, uint32_t n, const rayrs_camera* camera,
                       const rayrs_render_params* params, void* out_host, rayrs_render_stats* stats);

/* ---- tuning: the two scheduling choices a caller may legitimately make.  0 = the built-in default.  Neither changes
 * the arithmetic or the answer.  (Round 1 read such settings from RAYRS_* environment variables; a library must not.  The kernels'
 * development knobs -- thresholds, LDS budgets, test switches -- are not part of this boundary: rayrs_amd/csrc/rayrs_lab.h.) */
typedef struct {
    uint32_t pool_slots;    /* streaming route: paths in flight = slots of the pool in HBM, 128 + 33 bytes each
                               (default: min(items, 256 Mi, samples / 12)); ignored on the local-pool route */
    uint32_t local_pool;    /* a scene whose gate tree is at most one record (gate_n_wide <= 1: the reference's sphere
                               scenes) is rendered by ONE launch that keeps every path in LDS from its first ray
                               to its last (local_pool.hip) instead of three launches per bounce over a pool in
                               HBM; same arithmetic, same bits.  0 = do so, 1 = never (the streaming kernels) */
} rayrs_tuning;
/* Applies to the renders launched on this scene afterwards.  Waits for a render in flight. */
int rayrs_scene_set_tuning(rayrs_scene* scene, const rayrs_tuning* tuning);

/* ---- progressive film: the same block loop in passes.  A film is a device-resident accumulation buffer bound to one
 * scene, one camera and one set of sampling settings, to which samples are added pass by pass: look at a frame while it
 * converges, add samples to a frame that is still noisy without paying for the first ones again, stop when the noise
 * estimate says so, save a half-rendered frame and go on in another process.
 *
 * THE CONTRACT.  A sample's random numbers depend on (seed, pixel, sample index) only, and a pixel is the sum of its
 * per-chunk sums added in chunk order, the first one assigned.  So after passes n_1 ... n_k, N = n_1 + ... + n_k,
 * rayrs_film_read returns, bit for bit in both output formats, the frame rayrs_render returns for spp = N,
 * sample_chunk = c and the same seed, max_bounces, tile share and walk -- for every partition of N into passes that the
 * rules below allow, and across a rayrs_film_state_get / new film / rayrs_film_state_set in between.  The passes' rays
 * and paths add up to that frame's, and nan_pixels / neg_pixels of the status are that frame's.
 *   (rayrs_render with sample_chunk = 0 is the reference's ONE sequential sum per pixel, which no film reproduces in
 *   pieces: a film's frame is the sample_chunk = c frame.)
 *
 * RULES.
 *  - A film starts empty (N = 0).  c = sample_chunk is fixed for its life.  While the film is open N is a multiple of
 *    c.  A pass with n % c != 0 ends in a short chunk and CLOSES the film (a short chunk can only be the last chunk of
 *    the equivalent one-shot frame); n = 0, or any pass on a closed film, is RAYRS_INVALID_ARG and changes nothing.
 *  - N + n < 2^30 (a path's sample cursor has 30 bits: the limit of rayrs_render_params.spp), and a pass obeys the
 *    limits of a render of n samples (RAYRS_UNSUPPORTED: 2^32 (pixel, chunk) items, max_bounces > 8000, an image side
 *    > 65535).
 *  - A film holds a reference on nothing it does not own.  Destroying the scene before its films is the caller's
 *    error, as destroying it under a render in flight is.  A pass uses the scene's path pool, item sums and counters:
 *    one pass or one plain render in flight per scene (a pass waits for a rayrs_render_launch still in flight on the
 *    scene, as the next launch would); the calls on one scene and its films come from one thread at a time.
 *  - rayrs_render_multi does not take films.  A film with tile_rank / tile_ranks renders its share as rayrs_render
 *    does, which is what a caller with one process per GPU needs; pixels outside the share read as +0.
 *
 * NOISE.  A BATCH-MEANS estimate on c-sample batches -- the statistic the chunk sums support at no cost in the shading
 * kernels -- NOT a per-sample variance.  Per pixel, over the M full chunks so far (chunks of exactly c samples; M is
 * the same for every pixel), with y_k = (c_k.x + c_k.y) + c_k.z the channel sum of chunk sum k, the film keeps
 *     S1 = y_0 + y_1 + ...        S2 = y_0*y_0 + y_1*y_1 + ...
 * both accumulated in chunk order starting by assignment, unfused.  A pixel is CONVERGED AT tau iff
 *     M >= 2  and  M*S2 - S1*S1 <= ((tau*tau) * (S1*S1)) * (M-1)
 * evaluated in f64 in exactly this order, M converted to f64: the standard error of the mean of the chunk means,
 * estimated from their sample variance, is at most tau times the mean.  No square root and no division, so the count
 * is exactly reproducible.  A pixel whose S1 or S2 is not finite counts in `nonfinite` and not in `unconverged`;
 * `unconverged` = the pixels of the film's share that are neither converged nor non-finite.  With M < 2 every finite
 * pixel is unconverged.
 *
 * ADAPTIVE PASSES.  The film keeps a sample count N_t per 8x8 tile of the frame (the tile is the unit of a tile share and
 * of the film's records), and rayrs_film_render_adaptive adds samples only to the tiles that are still noisy.  THE
 * CONTRACT PER TILE: after any sequence of passes, the pixels of tile t that rayrs_film_read returns are, bit for bit in
 * both formats, the pixels rayrs_render returns for spp = N_t, sample_chunk = c and the same seed, max_bounces, tile
 * share and walk -- a tile may stop at its own sample count because of the two facts THE CONTRACT above rests on.
 * SELECTION: a pass of n samples takes tile t of the share iff N_t + n <= max_tile_samples and at least one pixel of the
 * tile inside the image is unconverged at tau by NOISE above, with M = M_t = N_t / c, the tile's own full chunks; a
 * non-finite pixel keeps no tile active, and neither does the padding of an edge tile.  The selected tiles are sampled
 * in ascending tile order, so a pass's work is a function of the film's state alone.
 *   On a film whose tiles differ: the status's noise counts use each tile's own M_t in the same predicate;
 * rayrs_film_status.samples is the largest N_t and full_chunks that divided by c; rays and paths stay the sums over
 * all passes; nan_pixels and neg_pixels are of the running sums as they stand; rayrs_film_read divides tile t by N_t.
 * rayrs_film_render(film, n) adds n samples to every tile from its own N_t, closes the film if n % c != 0, and its limit
 * is (largest N_t) + n < 2^30.  A film that only ever saw passes that took every tile behaves exactly as one that saw
 * rayrs_film_render alone. */
typedef struct rayrs_film rayrs_film;

typedef struct {            /* zero-initialise */
    uint32_t sample_chunk;  /* c >= 1, fixed for the film's life; 0 = 4 */
    uint32_t max_bounces;   /* main.rs:77 passes 50 */
    uint64_t seed;
    uint32_t tile_rank, tile_ranks; /* as rayrs_render_params; 0, 0 = 0, 1 */
    uint32_t fast_traversal;        /* as rayrs_render_params */
    uint32_t pad;
} rayrs_film_params;

typedef struct {
    uint64_t samples;       /* N: samples per pixel accumulated so far */
    uint64_t full_chunks;   /* M: chunks of exactly c samples among them */
    uint64_t rays, paths;   /* summed over all passes */
    uint64_t nan_pixels, neg_pixels; /* of the running sums as they stand (main.rs:81-87) */
    uint64_t unconverged, nonfinite; /* NOISE above, for the tau of the call */
    uint32_t closed;        /* 1 = the last pass ended in a short chunk: no further pass is accepted */
    uint32_t pad;
} rayrs_film_status;

/* RAYRS_NO_DEVICE on a host-only scene.  The film's footprint on the device: 40 bytes per pixel of the frame's 8x8 tiles. */
int rayrs_film_create(rayrs_scene* scene, const rayrs_camera* camera, const rayrs_film_params* params, rayrs_film** out);
void rayrs_film_destroy(rayrs_film* film);
/* Adds the samples N .. N+n-1 to every pixel of the film's share.  Synchronous.  pass_stats (may be NULL): as
 * rayrs_render's, for this pass alone (its nan_pixels / neg_pixels are 0: they are the status's). */
int rayrs_film_render(rayrs_film* film, uint32_t n, rayrs_render_stats* pass_stats);
/* Selects the tiles of the film's share with N_t + n <= max_tile_samples (0 = no cap but the 30-bit cursor) in which at
 * least one in-image pixel is unconverged at tau (NOISE, with M = N_t / c), and adds the samples N_t .. N_t + n - 1 to
 * every pixel of each selected tile.  n > 0 and n % c == 0 (an adaptive pass never closes a film); a closed film, a bad
 * tau or n: RAYRS_INVALID_ARG, nothing changes.  *active_tiles = the number selected; 0 is RAYRS_OK with no launch and
 * pass_stats zeroed.  On an empty film every tile is selected (M = 0: every finite pixel is unconverged).  Synchronous;
 * active_tiles and pass_stats may be NULL. */
int rayrs_film_render_adaptive(rayrs_film* film, uint32_t n, double tau, uint32_t max_tile_samples,
                               uint64_t* active_tiles, rayrs_render_stats* pass_stats);
/* N_t for the tiles_x * tiles_y tiles of the frame (tiles_x = ceil(x_pixels / 8)), row-major; 0 for tiles outside the
 * share.  Returns the number of tiles; writes min(that, cap). */
uint64_t rayrs_film_tile_samples(rayrs_film* film, uint32_t* out, uint64_t cap);
/* The frame as it stands: running sum * (1 / N) as RAYRS_OUT_F32 or RAYRS_OUT_F64 into a HOST buffer of
 * y_pixels*x_pixels*3 elements.  RAYRS_INVALID_ARG on an empty film. */
int rayrs_film_read(rayrs_film* film, uint32_t out_format, void* out_host);
/* tau: finite and >= 0. */
int rayrs_film_status_get(rayrs_film* film, double tau, rayrs_film_status* out);
/* Checkpoint: an opaque, versioned byte image of the film -- sums, statistics, counters, the per-tile sample counts (4
 * bytes per tile of the frame; image version 2, images of version 1 are refused) and the settings it was created with.  rayrs_film_state_set accepts only an image of this library's image version whose recorded image size, c, seed,
 * max_bounces, tile share and walk equal the film's, and whose length is exactly rayrs_film_state_bytes; otherwise
 * RAYRS_INVALID_ARG and the film is unchanged.  The scene and the camera themselves are NOT recorded: continuing on
 * another scene or view is the caller's error. */
uint64_t rayrs_film_state_bytes(const rayrs_film* film);
int rayrs_film_state_get(rayrs_film* film, void* out_host, uint64_t cap);
int rayrs_film_state_set(rayrs_film* film, const void* in_host, uint64_t bytes);

/* ---- first-hit feature buffers and a feature-guided denoiser: something to look at while a film converges, and the
 * depth / normal / albedo / object planes external denoisers and compositing want.  Neither touches a path kernel: the
 * features of a sample depend on (scene, camera, seed, pixel, sample index) only, so a kernel of their own recomputes them.
 *
 * FEATURES.  For pixel (row, col) and sample index s the primary ray is made exactly as a render makes it -- the path key
 * of (seed, pixel, s), then Camera::generate_primary_ray (lib.rs:202) with the render's flipped indices -- and the scene is
 * queried ONCE with z_near, z_far and the requested walk (the camera rule of rayrs_render_params.fast_traversal applies as
 * it does for a render).  Per-sample values on a hit of object obj at t:
 *     coverage_s = 1.0      depth_s = t
 *     normal_s   = obj.geom.normal(r.point(t)): what radiance hands to Material::evaluate (lib.rs:528-529), NOT flipped
 *                  towards the viewer
 *     albedo_s   = the rayrs_material.color the object was created with; (0,0,0) for RAYRS_MAT_NO_REFLECT
 * and on a miss all four are +0.  Per pixel and plane the sum over s = 0 .. F-1 is SEQUENTIAL, in sample order, the first
 * value assigned and the rest added, f64, unfused; the output is sum * (1.0 / (double)F).  (A sequential sum: there is no
 * chunk rule.)  The `object` plane (u32) holds the object hit by SAMPLE 0, in insertion order as rayrs_scene_export_bvh's
 * prim_object numbers them; a miss is 0xFFFFFFFF.  Pixels outside a tile share read +0 and 0xFFFFFFFF.
 *
 * DENOISER.  An edge-avoiding a-trous filter (Dammertz et al. 2010), specified to the operation.  Inputs per pixel: colour
 * c (3 f64), normal n, albedo a, depth z; scalars: L levels and kn, ka, kz, kc >= 0, the reciprocals of squared sigmas (the
 * filter never divides by a sigma); constants h[0] = 3/8, h[1] = 1/4, h[2] = 1/16.  Level k = 0 .. L-1 has step 2^k and
 * kc_k = kc * 4^k, formed on the host, reads the colour of level k-1 (level 0: the input) and the same features.  For pixel
 * p = (y, x):
 *   - if a component of c_p is not finite, c'_p = c_p;
 *   - else num = (0,0,0), den = 0, and for dy = -2 .. 2 (outer), dx = -2 .. 2 (inner), q = (y + dy*step, x + dx*step):
 *       skip q if it lies outside the image; skip q if a component of c_q is not finite;
 *       dn = ((n_p.x-n_q.x)^2 + (n_p.y-n_q.y)^2) + (n_p.z-n_q.z)^2, da likewise on a, dc likewise on this level's c,
 *       dz = (z_p-z_q)*(z_p-z_q);
 *       e = ((dn*kn + da*ka) + dz*kz) + dc*kc_k;   skip q if e is not finite;
 *       w = (h[|dy|]*h[|dx|]) * rr_exp(-e)   (include/rayrs_numeric.h);
 *       num += c_q * w per component (the product first, then the sum); den += w;
 *   - if den == 0 (the pixel's own features are NaN), c'_p = c_p; else c'_p = num / den, an f64 division per component.
 * A feature plane that is absent (NULL) contributes no term.  No albedo demodulation, nothing temporal (that is TEMPORAL ACCUMULATION below); the weight that is
 * guided by the film's own noise estimate is the GUIDED FILTER below.
 *
 * Refusals, all decided before the device is touched: RAYRS_INVALID_ARG for samples = 0 or >= 2^30, levels outside 1 .. 16,
 * a k that is negative or not finite, fast_traversal > 1, a bad tile share, rayrs_film_denoise on an empty film or on a film
 * with tile_ranks > 1 (the filter needs a pixel's neighbours); RAYRS_UNSUPPORTED for an image side > 65535; then
 * RAYRS_NO_DEVICE for a host-only scene. */

/* planes may be NULL = not wanted; host buffers; normal, albedo: H*W*3 f64, depth, coverage: H*W f64, object: H*W u32 */
int rayrs_render_features(rayrs_scene* scene, const rayrs_camera* camera, uint32_t samples, uint64_t seed, uint32_t tile_rank,
                          uint32_t tile_ranks, uint32_t fast_traversal, double* normal, double* albedo, double* depth,
                          double* coverage, uint32_t* object);
/* The same with the film's camera, seed, share and walk; independent of how many samples the film holds.  A film keeps the
 * features it made last on the device (8 doubles and a word per pixel), keyed by `samples`; the checkpoint image carries
 * none of it, and neither this call nor rayrs_film_denoise changes anything a later pass, rayrs_film_read,
 * rayrs_film_status_get or rayrs_film_state_get returns. */
int rayrs_film_features(rayrs_film* film, uint32_t samples, double* normal, double* albedo, double* depth, double* coverage,
                        uint32_t* object);
/* The frame rayrs_film_read(RAYRS_OUT_F64) returns, filtered on the device with the normal, albedo and depth of
 * `feature_samples` samples; out_host as rayrs_film_read's, RAYRS_OUT_F32 being the f64 result converted at the store. */
int rayrs_film_denoise(rayrs_film* film, uint32_t feature_samples, uint32_t levels, double kn, double ka, double kz, double kc,
                       uint32_t out_format, void* out_host);
/* The filter alone, on any frame, on HIP device `device`: host f64 buffers (color, out: h*w*3; normal, albedo: h*w*3;
 * depth: h*w), feature planes may be NULL. */
int rayrs_image_denoise(int device, uint32_t w, uint32_t h, const double* color, const double* normal, const double* albedo,
                        const double* depth, uint32_t levels, double kn, double ka, double kz, double kc, double* out);

/* ---- the film's noise estimate per pixel, and an a-trous filter guided by it: the spatial half of SVGF (Schied et al.
 * 2017).  The film's tiles differ in noise by construction after adaptive passes; here a tap's luminance difference is
 * divided by the pixel's own estimated standard deviation, and the variance is carried through the levels so that later
 * levels know how much noise is left.  Nothing here touches a path kernel, and there is no albedo demodulation.
 *
 * NOISE PLANE.  For pixel p in tile t of the film's share, with c the film's chunk, M = N_t / c (integer division) and
 * m = (double)M, S1 and S2 the pixel's sums of NOISE above:
 *   - outside the share: v = +0;
 *   - M < 2, or S1 or S2 not finite: v = +infinity -- selected, never computed: no NaN is ever generated, so the plane's
 *     bit patterns are comparable across machines;
 *   - otherwise d = m*S2 - S1*S1; if d is not finite, v = +infinity; else if !(d > 0), v = +0; else
 *       v = d / (((m*m)*(m-1.0)) * ((double)c*(double)c))
 *     one f64 division, unfused, in this order.
 * This is the batch-means variance of Y = (r+g)+b of the frame rayrs_film_read returns: the sample variance of the M chunk
 * sums, over M for their mean, over c*c for the per-sample scale.  On a CLOSED film the short last chunk is in the mean
 * (the frame) and not in the variance (S1, S2 and M count full chunks only).
 *
 * GUIDED FILTER.  Inputs per pixel: colour c (3 f64), variance v (1 f64: the variance of Y(c) = (c.x+c.y)+c.z), and the
 * optional normal n, albedo a, depth z exactly as DENOISER has them; scalars: L levels and kn, ka, kz, kv >= 0; constants
 * h[0] = 3/8, h[1] = 1/4, h[2] = 1/16, g[0] = 1/2, g[1] = 1/4 and RAYRS_GUIDED_EPS = 2^-33.  Level k = 0 .. L-1 has step
 * 2^k and reads the colour AND the variance of level k-1 (level 0: the inputs) and the same features.  For pixel p = (y, x):
 *   - if a component of c_p is not finite, c'_p = c_p and v'_p = v_p;
 *   - else the prefiltered variance, over the 3 x 3 ADJACENT pixels (distance 1, not step): gs = 0, gw = 0, and for
 *     dy = -1 .. 1 (outer), dx = -1 .. 1 (inner), q = (y + dy, x + dx):
 *       skip q if it lies outside the image; skip q if a component of c_q is not finite; skip q unless v_q >= 0 (which
 *       drops NaN and negatives and keeps +infinity);
 *       wt = g[|dy|]*g[|dx|];  gs += v_q*wt;  gw += wt;
 *     r_p = (gw == 0) ? +0 : kv / (gs/gw + RAYRS_GUIDED_EPS) -- two divisions per pixel and level, none per tap;
 *   - Yp = (c_p.x+c_p.y)+c_p.z, num = (0,0,0), den = 0, vs = 0, and for dy = -2 .. 2 (outer), dx = -2 .. 2 (inner),
 *     q = (y + dy*step, x + dx*step), the DENOISER order:
 *       skip q if it lies outside the image; skip q if a component of c_q is not finite; skip q unless v_q >= 0;
 *       dn, da, dz as DENOISER's;  Yq = (c_q.x+c_q.y)+c_q.z;  dl = Yp - Yq;
 *       e = ((dn*kn + da*ka) + dz*kz) + (dl*dl)*r_p;   skip q if e is not finite;
 *       w = (h[|dy|]*h[|dx|]) * rr_exp(-e);
 *       num += c_q * w per component (the product first, then the sum); den += w;
 *       ww = w*w;  vs += (ww == 0) ? +0 : v_q*ww   (the guard keeps 0 * infinity out);
 *   - if den == 0 or den*den == 0, c'_p = c_p and v'_p = v_p; else c'_p = num / den per component and
 *     v'_p = vs / (den*den).
 * An absent feature plane contributes no term; there is no kc.  Two consequences: where every variance is +infinity,
 * r_p = +0 everywhere and the colour output is, bit for bit, DENOISER's with kc = 0 -- so a film with fewer than two full
 * chunks falls back to the purely feature-guided filter; and on a flat frame with uniform variance and no features one
 * level multiplies an interior pixel's variance by (70/256)^2, the sum of the squared 5 x 5 weights.
 *
 * Refusals mirror rayrs_film_denoise and rayrs_image_denoise and are decided before the device is touched:
 * RAYRS_INVALID_ARG for levels outside 1 .. 16, a k that is negative or not finite, a NULL colour, variance or out, an
 * empty image, an empty film, a bad out_format, and for the filter on a film with tile_ranks > 1 (rayrs_film_noise accepts
 * a share); RAYRS_UNSUPPORTED for an image side > 65535; then RAYRS_NO_DEVICE.  Neither film call changes anything a
 * later pass, rayrs_film_read, rayrs_film_status_get or rayrs_film_state_get returns. */
#define RAYRS_GUIDED_EPS 0x1p-33

/* NOISE PLANE into a host buffer of y_pixels*x_pixels f64, row-major.  RAYRS_INVALID_ARG on an empty film. */
int rayrs_film_noise(rayrs_film* film, double* variance_host);
/* The frame rayrs_film_read(RAYRS_OUT_F64) returns and the plane rayrs_film_noise returns through GUIDED FILTER on the
 * device, with the features of `feature_samples` samples; out_host as rayrs_film_denoise's; out_variance (may be NULL):
 * the last level's variance, H*W f64. */
int rayrs_film_denoise_guided(rayrs_film* film, uint32_t feature_samples, uint32_t levels, double kn, double ka, double kz,
                              double kv, uint32_t out_format, void* out_host, double* out_variance);
/* The filter alone, on any frame, on HIP device `device`: host f64 buffers (color, out: h*w*3; variance: h*w; normal,
 * albedo: h*w*3; depth: h*w); feature planes and out_variance (h*w) may be NULL. */
int rayrs_image_denoise_guided(int device, uint32_t w, uint32_t h, const double* color, const double* variance,
                               const double* normal, const double* albedo, const double* depth, uint32_t levels,
                               double kn, double ka, double kz, double kv, double* out, double* out_variance);

/* ---- temporal accumulation: a history of what earlier views have seen, reprojected into each new view and blended with its
 * frame -- the temporal half of SVGF (Schied et al. 2017), where GUIDED FILTER above is the spatial half.  A film is bound to
 * one camera; a history carries the samples of a static scene from one camera to the next, so that a turntable or a
 * fly-through at 16 samples a frame shows more than 16 samples a frame.  Nothing here touches a path kernel or a film's state.
 *
 * TEMPORAL ACCUMULATION, specified to the operation.  A VIEW is a rayrs_camera and planes over its H x W pixels
 * (H = y_pixels, W = x_pixels, row-major, origin upper left): colour c (3 f64), variance v (of (c.x+c.y)+c.z, as GUIDED FILTER
 * has it), weight m (f64: how many samples the pixel stands for), and FEATURES' normal n, albedo a, depth z, coverage k,
 * object o.  The history is a view B (primed below), the incoming frame a view A whose weight plane is wc; the scalars are
 * max_weight > 0, tz2 = depth_tol*depth_tol and tn2 = normal_tol*normal_tol, formed on the host.  Ray::direction is not
 * normalised (lib.rs:31) and e_x, e_y are perpendicular to z (lib.rs:117-131), so a primary hit's t is its planar view depth
 * over |z| whatever the jitter, and with T the mean hit t the world point of a pixel centre is origin + T*(z + x*e_x + y*e_y):
 * the reprojection needs no square root and no elementary function.  For pixel p = (r, col) of A every expression is f64,
 * unfused, in the order written, and every condition is written in its positive form, so that a NaN takes the "no" side.
 * "No history" means out = (c_p, v_p, wc_p).  dot(a,b) = (a.x*b.x + a.y*b.y) + a.z*b.z.
 *   1. Pass-through.  If a component of c_p is not finite, or not wc_p > 0: out colour = c_p, out variance = v_p, out
 *      weight = wc_p if wc_p > 0, else +0.  (This step comes first on an empty history too.)
 *   2. The centre ray of the pixel, the render's flipped indices (main.rs:74-75) with the jitter replaced by 0.5:
 *        x = ((double)(W - col) + 0.5) / (double)ppc - width/2.
 *        y = ((double)(H - r) + 0.5) / (double)ppc - height/2.
 *        d = (z_cam + x*e_x) + y*e_y   per component, as lib.rs:209 forms it.
 *   3. The source vector.  If k_p > 0 (a hit pixel): T = z_p / k_p, P = origin_A + d*T, u = P - origin_B.  If k_p == 0
 *      (background: the environment is at infinity, only the direction matters): u = d.  Otherwise: no history.
 *   4. Into B.  s = dot(u, z'), zz = dot(z', z').  No history unless s > 0.  tp = s/zz,
 *        xp = (dot(u,e_x')*zz)/s,  yp = (dot(u,e_y')*zz)/s,
 *        fx = ((double)W' + 0.5) - (xp + width'/2.)*(double)ppc'
 *        fy = ((double)H' + 0.5) - (yp + height'/2.)*(double)ppc'
 *      (fx == col' is the centre of column col').  No history unless fx >= -1 && fx < W' && fy >= -1 && fy < H'.
 *      x0 = floor(fx), ax = fx - x0; y0, ay likewise.
 *   5. The taps.  bs = 0, hc = (0,0,0), hv = 0, hm = 0, and for j = 0,1 (outer), i = 0,1 (inner), q = (y0+j, x0+i),
 *      b = (i ? ax : 1-ax) * (j ? ay : 1-ay):  skip q if it lies outside B; if b == 0; if a component of c'_q is not finite; if
 *      not v'_q >= 0; if not m'_q > 0; if it is not geometrically valid -- for a background p: k'_q == 0; for a hit p all of
 *        k'_q > 0 and o'_q == o_p;
 *        with Tq = z'_q/k'_q and dt = Tq - tp:  dt*dt <= tz2*(tp*tp);
 *        ((n_p.x-n'_q.x)^2 + (n_p.y-n'_q.y)^2) + (n_p.z-n'_q.z)^2 <= tn2.
 *      (Each is a plain skip: the order they are tried in changes no result.)  For a valid tap
 *        bs += b;  hc += c'_q*b per component (the product first);  hv += v'_q*b;  hm += m'_q*b.
 *      The variance is interpolated linearly: an upper bound under full correlation, which is the case for neighbouring taps
 *      of a filtered history.
 *   6. If bs == 0 (no valid tap): no history.
 *   7. C = hc/bs per component, V = hv/bs, M0 = hm/bs, M = (M0 < max_weight) ? M0 : max_weight.
 *   8. Healing -- a frame with fewer than two chunks must not poison a static view for ever:
 *        vp = (v_p >= 0) ? v_p : +infinity;
 *        if vp == +infinity and V < +infinity:  vp = (V*M0)/wc_p;  else if V == +infinity and vp < +infinity:  V = (vp*wc_p)/M0.
 *   9. The blend.  alpha = wc_p/(wc_p + M), beta = 1 - alpha;
 *        out colour = C*beta + c_p*alpha per component (two products, then the sum);
 *        out variance = tb + ta,  tb = (beta*beta == 0) ? +0 : V*(beta*beta),  ta = (alpha*alpha == 0) ? +0 : vp*(alpha*alpha);
 *        out weight = M + wc_p.
 *  10. After the push the history's camera and feature planes are A's, unchanged; its colour, variance and weight are the
 *      outputs.  A push into an empty history is step 1, and "no history" for every other pixel.  B's size may differ from A's.
 * KNOWN LIMIT.  What is reprojected is the first hit: reflections and refractions in mirror and glass objects move with the
 * surface that shows them and lag behind the view.  max_weight bounds the lag (alpha >= wc/(wc + max_weight)).
 *
 * ORBIT.  rayrs_camera_orbit turns `origin` by `degrees` about the axis through `lookat` along `up` (Rodrigues' rotation) with
 * rr_sin / rr_cos of include/rayrs_numeric.h, so that every caller builds the same cameras to the bit:
 *     n2 = (up.x*up.x + up.y*up.y) + up.z*up.z;  inv = 1.0/rr_sqrt(n2);  k = up*inv;  v = origin - lookat;
 *     rad = degrees * (RR_PI/180.0);  c = rr_cos(rad);  s = rr_sin(rad);
 *     kv = (k.x*v.x + k.y*v.y) + k.z*v.z;  g = kv*(1.0 - c);
 *     x = (k.y*v.z - k.z*v.y, k.z*v.x - k.x*v.z, k.x*v.y - k.y*v.x);
 *     out = lookat + ((v*c + x*s) + k*g)   per component;
 * degrees == 0 returns `origin` itself, bit for bit, so that the first frame of an orbit is the frame of the camera as given.
 * RAYRS_INVALID_ARG for a null pointer, degrees that are not finite, an `up` whose n2 is not > 0 or not finite.
 *
 * Refusals, all decided before the device is touched, mirroring rayrs_film_denoise_guided: RAYRS_INVALID_ARG for a NULL
 * required plane, an empty image, max_weight not > 0 or not finite, a negative or non-finite tolerance, a bad out_format,
 * levels or k as DENOISER has them, an empty film, a film with tile_ranks > 1, a film on another device than the history, a
 * read or a filter on an empty history; RAYRS_UNSUPPORTED for an image side > 65535; then RAYRS_NO_DEVICE (a history made
 * with device = -1).  Neither film call changes anything a later pass, rayrs_film_read, rayrs_film_status_get or
 * rayrs_film_state_get returns.  The calls on one history, and on the film it is handed, come from one thread at a time. */
typedef struct rayrs_history rayrs_history;

/* An empty history on HIP device `device`, which is first touched by a push. */
int rayrs_history_create(int device, rayrs_history** out);
void rayrs_history_destroy(rayrs_history* history);
/* Empties the history; its buffers are kept. */
int rayrs_history_reset(rayrs_history* history);
/* Pushes a view of the caller's: host planes of the camera's H x W pixels -- color, normal, albedo: H*W*3 f64; variance,
 * weight, depth, coverage: H*W f64; object: H*W u32.  albedo may be NULL: it is only carried for the filter, which then has
 * no albedo term. */
int rayrs_history_push_image(rayrs_history* history, const rayrs_camera* camera, const double* color, const double* variance,
                             const double* weight, const double* normal, const double* albedo, const double* depth,
                             const double* coverage, const uint32_t* object, double max_weight, double depth_tol,
                             double normal_tol);
/* Pushes the film as it stands, everything staying on the device: the frame rayrs_film_read(RAYRS_OUT_F64) returns, the plane
 * rayrs_film_noise returns, weight = (double)N_t of the pixel's tile, and the film's features of `feature_samples` samples
 * (the object plane as rayrs_film_features numbers it). */
int rayrs_history_push_film(rayrs_history* history, rayrs_film* film, uint32_t feature_samples, double max_weight,
                            double depth_tol, double normal_tol);
/* HIP-event times of the last push, if it was a rayrs_history_push_film (else RAYRS_INVALID_ARG), in milliseconds: the
 * features pass (0 if the film held them), the frame, the noise plane, the copies of the features into the history, the
 * reprojection. */
int rayrs_history_push_times(rayrs_history* history, double ms[5]);
/* The history's colour (H*W*3), variance and weight (H*W each) into host buffers, each of which may be NULL; RAYRS_OUT_F64,
 * or RAYRS_OUT_F32: every f64 value converted.  RAYRS_INVALID_ARG on an empty history. */
int rayrs_history_read(rayrs_history* history, uint32_t out_format, void* color, void* variance, void* weight);
/* GUIDED FILTER on the history's colour and variance with its current normal, albedo and depth planes; out_host and
 * out_variance as rayrs_film_denoise_guided's. */
int rayrs_history_denoise_guided(rayrs_history* history, uint32_t levels, double kn, double ka, double kz, double kv,
                                 uint32_t out_format, void* out_host, double* out_variance);
/* ORBIT above. */
int rayrs_camera_orbit(const double origin[3], const double up[3], const double lookat[3], double degrees, double out_origin[3]);

/* ---- ray queries: the scene asked about rays of the caller's -- picking, probes, baking, visibility, shadow and
 * ambient-occlusion rays -- in batches, on the host or on device-resident buffers on a stream.  Nothing here touches a path
 * kernel, a film or a render's buffers: the kernels are a unit of their own (query.hip).
 *
 * RAY QUERIES, specified to the operation.  A ray is (o, d), three f64 each, USED AS GIVEN: Ray::direction is not normalised
 * (lib.rs:31), so t is in units of |d|.  Any f64 is a legal component -- NaN, infinities, a zero direction: the walk treats
 * them as the reference's arithmetic does.
 *
 * CLOSEST HIT (rayrs_scene_intersect).  The query is the render's: Bvh::intersect (bvh.rs:212-214, :391-415) with the scene's
 * z_near, z_far.  fast_traversal = 0 takes the default walk of rayrs_render_params.fast_traversal, the reference's visit set
 * by construction; fast_traversal = 1 takes the fast walk with both of its bets.  There is no camera here, so the camera rule
 * does not apply: fast_traversal = 1 is taken AS ASKED, and the rule's caveat -- from far away the leaf-box bet fails for
 * about one in-plane ray in 10^4 -- applies to the caller's rays, whose origins the library does not look at.  Per ray, on a
 * hit of object obj at t:
 *     t      = t (f64)
 *     object = obj (u32), in insertion order as rayrs_scene_export_bvh's prim_object numbers them
 *     normal = FEATURES' normal_s: obj.geom.normal(r.point(t)), what radiance hands to Material::evaluate (lib.rs:528-529),
 *              NOT flipped towards the ray's origin; 3 f64; the buffer may be NULL = not wanted
 * and on a miss t = +0, object = 0xFFFFFFFF, normal = (+0, +0, +0).
 *
 * OCCLUSION (rayrs_scene_occluded).  occluded_i = 1 iff the closest-hit query above finds a hit and t < t_max_i, else 0;
 * one uint8_t per ray.  The condition is in its positive form, so a NaN, zero or negative t_max gives 0; t_max == NULL means
 * +infinity for every ray.  t_max is never handed to a box test or to the accept rule: the visit set and the acceptance window
 * stay (z_near, z_far), which keeps the verdict a function of the closest-hit answer alone.  The walk behind it is an ANY-HIT
 * walk: it culls nothing, so which primitives a ray is tested of is decided by the boxes alone and the closest hit is among
 * them; an accepted t < t_max anywhere in that set implies the closest is < t_max, in any visiting order -- so a ray stops at
 * the first such hit instead of paying for its whole visit set.  fast_traversal = 0: the default walk's trees (the verdict is
 * the reference's for every ray by construction).  fast_traversal = 1: the tree of single primitives behind their own boxes
 * (rayrs_scene_export_wide) with NOTHING CULLED and the same early exit -- the leaf-box bet WITHOUT the culling bet; its
 * verdict is "a hit with t < t_max over that tree's visit set".
 *
 * The first two entry points take HOST buffers and are synchronous.  The _launch forms take DEVICE pointers on the scene's
 * device and a hipStream_t (NULL = the default stream), enqueue and return without a host wait: what the caller enqueues on
 * the stream afterwards is ordered behind the query, as it is behind rayrs_render_launch.  A batch goes through launches of
 * at most 2^20 rays each.  After the first call of a given walk a _launch call allocates nothing.
 *
 * Refusals, all decided before the device is touched, in this order: RAYRS_INVALID_ARG for a NULL scene or a NULL required
 * buffer (origin, direction, t, object; origin, direction, occluded) -- with n == 0 too; RAYRS_INVALID_ARG for
 * fast_traversal > 1; RAYRS_NO_DEVICE for a host-only scene.  n == 0 on a device scene is RAYRS_OK and launches nothing.
 *
 * The calls on one scene come from one thread at a time.  A query owns its scratch (a strip for the traversal stacks' overflow,
 * which the scene keeps, and the host forms' staging buffers) and touches nothing of a render's: it is ordered against a
 * render in flight only by the streams.  Queries on one scene whose trees need the strip follow one another on the device
 * whichever streams they are given (the later one's stream waits for the earlier one; no host wait). */
int rayrs_scene_intersect(rayrs_scene* scene, const double* origin, const double* direction, uint64_t n, uint32_t fast_traversal,
                          double* t, uint32_t* object, double* normal /* may be NULL */);
int rayrs_scene_occluded(rayrs_scene* scene, const double* origin, const double* direction, const double* t_max /* may be NULL */,
                         uint64_t n, uint32_t fast_traversal, uint8_t* occluded);
int rayrs_scene_intersect_launch(rayrs_scene* scene, const double* origin, const double* direction, uint64_t n,
                                 uint32_t fast_traversal, double* t, uint32_t* object, double* normal /* may be NULL */,
                                 void* hip_stream);
int rayrs_scene_occluded_launch(rayrs_scene* scene, const double* origin, const double* direction,
                                const double* t_max /* may be NULL */, uint64_t n, uint32_t fast_traversal, uint8_t* occluded,
                                void* hip_stream);

/* ---- ambient occlusion: the consumer of the occlusion query above that the library can make the rays of itself -- a cosine
 * lobe of `samples` rays around each point's normal, counted.  Nothing here touches a path kernel, a film or a render's
 * buffers: the kernels are a unit of their own (ao.hip).
 *
 * AMBIENT OCCLUSION, specified to the operation.  A point is (p, n), three f64 each, USED AS GIVEN: the library does not
 * normalise or inspect them.  samples = S >= 1; t_max, bias: one f64 each for the call; seed, index_base: u64.  For point i
 * of the call and sample s in 0 .. S-1:
 *     key = rr_path_key(seed, index_base + i, s)                         (rayrs_numeric.h)
 *     u = rr_uniform(key, 0), v = rr_uniform(key, 1)
 *     (e1, e2) = onb(n_i)                                                (vecmath.rs:341-352)
 *     phi = 2.0 * RR_PI * v;  su = sqrt(u)
 *     l = (e1 * (cos(phi) * su) + e2 * (sin(phi) * su)) + n_i * sqrt(1.0 - u)
 *     o = p_i + n_i * bias
 *     occ = OCCLUSION(o, l, t_max)                                       (RAY QUERIES: the same rule and the same walks)
 * every operation f64 and unfused, in the operand and operation order of the reference's Lambertian scatter direction
 * (material.rs:259-281, :982-993): the directions are that material's, bit for bit, on two draws each.  Per point:
 *     count_i      = the number of samples with occ (u32)
 *     visibility_i = (double)(S - count_i) / (double)S, one true division (f64)
 * Either output buffer may be NULL = not wanted, but not both.  index_base makes a call on points[a:b] with index_base = a
 * return the slice of the whole call's answer.  A NaN, zero or negative t_max gives count 0, by OCCLUSION's positive form;
 * +infinity means anywhere.  fast_traversal means what it means for rayrs_scene_occluded.  The count is an integer sum, so it
 * is the same bits however the kernel schedules a point's samples.
 *
 * AMBIENT OCCLUSION PLANE (rayrs_render_ao).  For pixel (row, col) take sample 0's primary ray as FEATURES forms it --
 * sample_key(seed, cam, row, col, 0) and sample_ray -- and its closest hit by the render's query (the walk a render with
 * these settings takes).  On a miss count = 0 and visibility = 1.0, and no AO ray is traced.  On a hit at t: p = o + d * t;
 * n = FEATURES' normal_s turned against the ray (if n . d > 0.0 then n = n * -1.0); then the operation above at (p, n) with
 * index_base + i = row * W + col and seed ao_seed -- a parameter of its own: with the primary seed, sample 0's draws 0 and 1
 * would be the pixel jitter's.  The result is the whole frame's (H, W) planes in image order; there are no tile shares.
 *
 * rayrs_scene_ambient_occlusion takes HOST buffers and is synchronous, as rayrs_render_ao.  The _launch form takes DEVICE
 * pointers on the scene's device and a hipStream_t (NULL = the default stream), enqueues and returns without a host wait; after
 * the first call of a given walk it allocates nothing.  A batch goes through launches of at most 2^20 threads each, which share
 * RAY QUERIES' stack strip and its ordering rule.
 *
 * Refusals, all decided before the device is touched, in RAY QUERIES' order: RAYRS_INVALID_ARG for a NULL scene, a NULL
 * position or normal, both outputs NULL, samples == 0 or fast_traversal > 1 -- with n == 0 too; then RAYRS_NO_DEVICE for a
 * host-only scene.  n == 0 on a device scene is RAYRS_OK and launches nothing.  rayrs_render_ao refuses a NULL camera and the
 * cameras rayrs_render_features refuses, likewise before RAYRS_NO_DEVICE. */
int rayrs_scene_ambient_occlusion(rayrs_scene* scene, const double* position, const double* normal, uint64_t n, uint32_t samples,
                                  double t_max, double bias, uint64_t seed, uint64_t index_base, uint32_t fast_traversal,
                                  uint32_t* count /* may be NULL */, double* visibility /* may be NULL */);
int rayrs_scene_ambient_occlusion_launch(rayrs_scene* scene, const double* position, const double* normal, uint64_t n,
                                         uint32_t samples, double t_max, double bias, uint64_t seed, uint64_t index_base,
                                         uint32_t fast_traversal, uint32_t* count /* may be NULL */,
                                         double* visibility /* may be NULL */, void* hip_stream);
int rayrs_render_ao(rayrs_scene* scene, const rayrs_camera* camera, uint64_t seed, uint64_t ao_seed, uint32_t samples, double t_max,
                    double bias, uint32_t fast_traversal, uint32_t* count /* may be NULL */, double* visibility /* may be NULL */);

/* ---- radiance queries: the light the render computes, along rays of the caller's and at points of the caller's -- an
 * environment probe, a camera model of the caller's own, irradiance at lightmap texels or probe positions -- in batches, on the
 * host or on device-resident buffers on a stream.  Nothing here touches a path kernel, a film or a render's buffers: the
 * kernels are a unit of their own (radiance.hip).
 *
 * RADIANCE QUERY, specified to the operation.  A ray is (o, d), three f64 each, USED AS GIVEN, as in RAY QUERIES.  samples =
 * S >= 1, max_bounces, sample_chunk = c: u32; seed, index_base: u64.  For ray i of the call and sample s in 0 .. S-1:
 *     key      = rr_path_key(seed, index_base + i, s);  rng = (key, draw 0)   (rayrs_numeric.h)
 *     L_{i,s}  = radiance(scene, Ray{o_i, d_i}, max_bounces)                  (lib.rs:521-560)
 * with the draws taken in program order from rng, and the loop's query the render's: Bvh::intersect with the scene's z_near,
 * z_far.  fast_traversal means what it means for rayrs_scene_intersect, and is taken AS ASKED: there is no camera for the
 * camera rule to look at.  Then, with c' = S if c == 0 or c >= S, else c, and chunk k = the samples k*c' .. min((k+1)*c', S) - 1:
 *     C_k        = Vec3::zeros(); C_k += L_{i,s} in sample order               (main.rs:67-69)
 *     sum_i      = C_0 assigned, then += C_k in chunk order                    (rayrs_render_params.sample_chunk's rule)
 *     radiance_i = sum_i * (1.0 / (double)S)                                   (main.rs:89; Div<f64> multiplies by the reciprocal)
 *     queries_i  = the number of Bvh::intersect calls of the ray's S paths (u32)
 * every operation f64 and unfused; radiance is 3 f64 per ray.  Either output buffer may be NULL = not wanted, but not both.
 * index_base makes a call on rays[a:b] with index_base = a return the slice of the whole call's answer.  max_bounces == 0 is
 * legal: the loop runs no turn, radiance is +0 and queries is 0.  No f64 sum depends on how the kernel schedules its lanes: a
 * chunk's sum is made in one lane in sample order, the rest by a resolve in chunk order.
 *
 * IRRADIANCE.  A point is (p, n), three f64 each, USED AS GIVEN, as in AMBIENT OCCLUSION; bias: one f64 for the call.  For point
 * i and sample s: key as above; draws 0 and 1 make l exactly as AMBIENT OCCLUSION does; o = p_i + n_i * bias; and
 *     L_{i,s} = radiance(scene, Ray{o, l}, max_bounces)    with the path's rng continuing at draw 2
 * which is what Material::evaluate of a Lambertian surface at (p, n) followed by the loop does with one rng.  The sums and the
 * outputs are the RADIANCE QUERY's.  The value is the cosine-weighted mean of the incoming radiance, E / pi: for the irradiance
 * E multiply by pi; a Lambertian texel of albedo rho radiates rho times the value.
 *
 * rayrs_scene_radiance and rayrs_scene_irradiance take HOST buffers and are synchronous.  The _launch forms take DEVICE
 * pointers on the scene's device and a hipStream_t (NULL = the default stream), enqueue and return without a host wait; after the
 * first call of a given walk a _launch call allocates nothing.  An item is (ray, chunk); a batch goes through launches of whole
 * rays, at most 2^20 items each, which share RAY QUERIES' stack strip and its ordering rule (and a scratch of the scene's under
 * the same rule).
 *
 * Refusals, all decided before the device is touched, in RAY QUERIES' order: RAYRS_INVALID_ARG for a NULL scene, a NULL
 * origin / direction (position / normal), both outputs NULL, samples == 0 or fast_traversal > 1 -- with n == 0 too; then
 * RAYRS_UNSUPPORTED for samples or max_bounces beyond the limits rayrs_render_params puts on spp and max_bounces (2^30 - 1;
 * 8000), for (uint64)samples * max_bounces >= 2^32 (queries_i could wrap), and for more than 2^20 chunks per ray (a launch
 * takes whole rays); then RAYRS_NO_DEVICE for a host-only scene.  n == 0 on a device scene is RAYRS_OK and launches nothing. */
int rayrs_scene_radiance(rayrs_scene* scene, const double* origin, const double* direction, uint64_t n, uint32_t samples,
                         uint32_t max_bounces, uint32_t sample_chunk, uint64_t seed, uint64_t index_base, uint32_t fast_traversal,
                         double* radiance /* may be NULL */, uint32_t* queries /* may be NULL */);
int rayrs_scene_radiance_launch(rayrs_scene* scene, const double* origin, const double* direction, uint64_t n, uint32_t samples,
                                uint32_t max_bounces, uint32_t sample_chunk, uint64_t seed, uint64_t index_base,
                                uint32_t fast_traversal, double* radiance /* may be NULL */, uint32_t* queries /* may be NULL */,
                                void* hip_stream);
int rayrs_scene_irradiance(rayrs_scene* scene, const double* position, const double* normal, uint64_t n, uint32_t samples,
                           uint32_t max_bounces, uint32_t sample_chunk, double bias, uint64_t seed, uint64_t index_base,
                           uint32_t fast_traversal, double* radiance /* may be NULL */, uint32_t* queries /* may be NULL */);
int rayrs_scene_irradiance_launch(rayrs_scene* scene, const double* position, const double* normal, uint64_t n, uint32_t samples,
                                  uint32_t max_bounces, uint32_t sample_chunk, double bias, uint64_t seed, uint64_t index_base,
                                  uint32_t fast_traversal, double* radiance /* may be NULL */, uint32_t* queries /* may be NULL */,
                                  void* hip_stream);

/* ---- radiance queries with light sampling: the queries above with the reference's Some(pdf) in place of None, and the same
 * loop over a camera's pixels.  The reference designed the mix (Material::evaluate takes an Option<Pdf>, material.rs:91-97;
 * LambertianDiffuse::scatter mixes it with its cosine lobe, :259-281; Plastic hands it to its diffuse arm, :588; the seven
 * other scatters ignore it) and its radiance() passes None (lib.rs:532): here the caller names the lights.  The kernels are a
 * unit of their own (radiance_lit.hip); nothing above changes, rayrs_render and the film know nothing of it.
 *
 * LIGHT SAMPLING, specified to the operation.  A LIGHT LIST is K <= RAYRS_MAX_LIGHTS object indices, in the numbering
 * rayrs_scene_intersect returns as `object` (insertion order, a mesh one index per triangle).  Each index must name a sphere or
 * a plane object; it need not emit (a portal is a legitimate target); duplicates are legal and mean what the density below
 * says.  K = 0 is pdf = None: every lit entry point then returns, bit for bit and count for count, what its unlit counterpart
 * returns.  With K >= 1, Material::evaluate of a LambertianDiffuse surface, and of Plastic's diffuse arm after Plastic's own
 * Fresnel draw, at (position, normal) with the surface's colour `albedo` is, the draws taken from the path's rng in this order:
 *     a = rng.next()
 *     if a < 0.5:                                   (Pdf::Mix::generate, material.rs:1028-1034, MixKind::Constant(0.5))
 *         b = rng.next();  k = min((uint32)(b * (double)K), K - 1)
 *         u1 = rng.next();  u2 = rng.next()
 *         q = light k's Hittable::sample:
 *             plane  (geometry.rs:288-299): u = u1 * (umax - umin) + umin;  v = u2 * (vmax - vmin) + vmin;
 *                    q = (pos, u, v) | (u, pos, v) | (u, v, pos) for an X | Y | Z axis
 *             sphere (geometry.rs:142-152): phi = 2.0 * RR_PI * u2;  r = sqrt(u1 * (1.0 - u1));
 *                    x = cos(phi) * 2.0 * r;  y = sin(phi) * 2.0 * r;  z = 1.0 - 2.0 * u1;
 *                    q = (x, y, z) * sqrt(radius2) + origin
 *         l = (q - position).unit()                 (material.rs:1027)
 *     else:
 *         l = Pdf::Cosine.generate                  (two draws: exactly the unlit Lambertian's direction, AMBIENT OCCLUSION's l)
 *     ndl = normal . l
 *     pdf = +inf if ndl < 0.0                       (material.rs:952-954)
 *           else 0.5 * p_L + 0.5 * (ndl * RR_FRAC_1_PI),
 *           p_L = (p_0 assigned, then += p_k in list order) / (double)K, one true division
 *     color = ((albedo * RR_FRAC_1_PI) * ndl) / pdf     (material.rs:273-274; Div<f64> multiplies by the reciprocal)
 *     Scatter { color, Ray(position, l) }
 * The light arm takes four draws and the cosine arm three; the loop's roulette draw follows as it does without lights.  The
 * other seven materials and Plastic's Cook-Torrance arm are unchanged, as in the reference.
 *
 * p_k(l) is the TRUE solid-angle density, at `position`, of the directions that light k's arm generates.  This is the one
 * place where the operation deliberately leaves the reference (Pdf::Hittable's value, material.rs:943-950): the estimator is
 * unbiased only if the density it divides by is the density it draws from, and the reference's is that in two cases out of
 * many -- it divides by the SHADING normal's n . l where the area's projection is the LIGHT's |n_k . l|, and of a sphere it
 * prices the near crossing only where uniform sampling of the sphere's area reaches its far side too.  With ray = Ray{position, l}:
 *     plane:  Plane::intersect(ray) (geometry.rs:229-271); if it is Some(t) and t > 0.0:
 *                 p_k = (position - ray.point(t)).mag2() / (|n_k . l| * area),  area = (umax - umin) * (vmax - vmin),
 *                 n_k = Plane::normal (geometry.rs:273-282), the dot product written out in full (three products, two sums);
 *             else p_k = 0.0
 *     sphere: odiff, a, b, c, desc of Sphere::intersect (geometry.rs:107-113); p_k = 0.0; if desc > 0.0:
 *                 t1 = (-b - sqrt(desc)) / (2.0 * a);  t2 = (-b + sqrt(desc)) / (2.0 * a)
 *                 if t1 > 0.0: p_k = p_k + X(t1);  if t2 > 0.0: p_k = p_k + X(t2)
 *                 X(t) = (position - ray.point(t)).mag2() / (|Sphere::normal(ray.point(t)) . l| * area),
 *                 area = (4.0 * RR_PI) * radius2
 * Everything is f64 and unfused; ray.point(t) = position + l * t; a zero or non-finite intermediate takes whatever IEEE gives
 * (q == position, a grazing |n_k . l| = 0, a point inside a sphere light).  Where pdf = +inf the densities are not evaluated.
 *
 * RADIANCE, LIT (rayrs_scene_radiance_lit): RADIANCE QUERY with the operation above in place of evaluate(.., None).
 * IRRADIANCE, LIT (rayrs_scene_irradiance_lit): with K >= 1 the sample's first direction comes from the same operation at
 * position = p_i + n_i * bias, normal n_i, albedo (1, 1, 1), on the path's rng from draw 0; then
 *     L_{i,s} = color * radiance(scene, Ray{position, l}, max_bounces)   componentwise, the path's rng continuing;
 * the path is traced whatever color is.  With K = 0 it is IRRADIANCE, with no multiplication.
 * IMAGE FORM (rayrs_render_lit): pixel (row, col) is ray i = row * W + col of an H * W batch; key = sample_key(seed, cam, row,
 * col, s) (= rr_path_key(seed, i, s)), the primary ray is the render's sample_ray on draws 0 and 1, the loop goes on at draw 2,
 * and the sums are RADIANCE QUERY's.  With K = 0 the frame is rayrs_render's with out_format = RAYRS_OUT_F64 and the same
 * sample_chunk, bit for bit: rayrs_render sums by the same rule and does nothing beyond it to an f64 frame (its NaN and
 * negative-pixel counters only count).  There are no tile shares.  fast_traversal is treated as rayrs_render_ao treats it: the
 * walk is the one a render with these settings takes (the camera rule of rayrs_render_params.fast_traversal included), for the
 * whole path; in the other four entry points it is taken as asked.
 *
 * `lights` is a HOST pointer in every form, the _launch forms included: the list is resolved on the host into a table of a
 * kind and seven f64 per light and passed by value in the kernel arguments, so a _launch call still allocates nothing (after
 * the first call of a given walk) and orders no copy.  Buffers, streams, launches and the stack strip are RADIANCE QUERY's.
 *
 * Refusals, all decided before the device is touched and with n == 0 too, in RADIANCE QUERY's order: to its RAYRS_INVALID_ARG
 * group add lights == NULL with n_lights > 0 and an index >= the scene's object count (rayrs_render_lit: a NULL camera or
 * out_rgb, and the cameras rayrs_render_features refuses as arguments); to its RAYRS_UNSUPPORTED group add n_lights >
 * RAYRS_MAX_LIGHTS and an index that names a triangle (rayrs_render_lit: an image side above 65535); RAYRS_NO_DEVICE last. */
#define RAYRS_MAX_LIGHTS 8
int rayrs_scene_radiance_lit(rayrs_scene* scene, const double* origin, const double* direction, uint64_t n, uint32_t samples,
                             uint32_t max_bounces, uint32_t sample_chunk, uint64_t seed, uint64_t index_base, uint32_t fast_traversal,
                             const uint32_t* lights, uint32_t n_lights, double* radiance /* may be NULL */,
                             uint32_t* queries /* may be NULL */);
int rayrs_scene_radiance_lit_launch(rayrs_scene* scene, const double* origin, const double* direction, uint64_t n, uint32_t samples,
                                    uint32_t max_bounces, uint32_t sample_chunk, uint64_t seed, uint64_t index_base,
                                    uint32_t fast_traversal, const uint32_t* lights, uint32_t n_lights,
                                    double* radiance /* may be NULL */, uint32_t* queries /* may be NULL */, void* hip_stream);
int rayrs_scene_irradiance_lit(rayrs_scene* scene, const double* position, const double* normal, uint64_t n, uint32_t samples,
                               uint32_t max_bounces, uint32_t sample_chunk, double bias, uint64_t seed, uint64_t index_base,
                               uint32_t fast_traversal, const uint32_t* lights, uint32_t n_lights,
                               double* radiance /* may be NULL */, uint32_t* queries /* may be NULL */);
int rayrs_scene_irradiance_lit_launch(rayrs_scene* scene, const double* position, const double* normal, uint64_t n, uint32_t samples,
                                      uint32_t max_bounces, uint32_t sample_chunk, double bias, uint64_t seed, uint64_t index_base,
                                      uint32_t fast_traversal, const uint32_t* lights, uint32_t n_lights,
                                      double* radiance /* may be NULL */, uint32_t* queries /* may be NULL */, void* hip_stream);
int rayrs_render_lit(rayrs_scene* scene, const rayrs_camera* camera, uint64_t seed, uint32_t samples, uint32_t max_bounces,
                     uint32_t sample_chunk, uint32_t fast_traversal, const uint32_t* lights, uint32_t n_lights,
                     double* out_rgb /* H*W*3 */, uint32_t* queries /* H*W, may be NULL */);

/* ---- radiance queries with direct lighting: a third strategy beside the unlit queries and LIGHT SAMPLING, in the same three
 * forms.  A diffuse bounce keeps the direction the surface itself samples and sends a second, cheap ray towards a sampled point
 * of a light (next-event estimation); the two are weighted against each other by the balance heuristic (multiple importance
 * sampling).  Where the lamps matter little the light sample adds little and everything else keeps weight 1; where a lamp
 * dominates, every bounce finds it; and no quotient can be 0 / 0.  The kernels are a unit of their own (radiance_direct.hip);
 * nothing above changes.
 *
 * DIRECT LIGHTING, specified to the operation.  The light list is LIGHT SAMPLING's: K <= RAYRS_MAX_LIGHTS object indices,
 * spheres and planes, duplicates legal.  Everything is f64 and unfused; the draws are taken from the path's rng in program
 * order; p_k, p_L = (p_0 assigned, then += p_k in list order) / (double)K, light k's Hittable::sample and the list's numbering
 * are LIGHT SAMPLING's, unchanged.  "obj is in the list" is set membership: obj's index equals some entry's.
 *
 * State.  A path carries one extra scalar w, the weight of the emission of a LISTED object met by the current ray: w = 1.0 at a
 * path's start, and w = 1.0 after every bounce that is not a diffuse bounce.
 *
 * One turn of radiance()'s loop at a hit obj (lib.rs:526-551), K >= 1:
 *     ev = Material::evaluate(position, normal, view, None)       exactly the unlit call, its draws unchanged
 *     if NoScatter: return light
 *     e = obj.emission.emit();  if obj is in the list: e = e * w
 *     light = light + throughput * e
 *     diffuse = obj.mat is LambertianDiffuse, or Plastic whose Fresnel draw chose the diffuse arm (material.rs:587-588)
 *     if diffuse:                                                 (albedo = the material's colour)
 *         b = rng.next();  u1 = rng.next();  u2 = rng.next()      always three draws, after evaluate's own
 *         k = min((uint32)(b * (double)K), K - 1);  q = light k's Hittable::sample(u1, u2);  l_s = (q - position).unit()
 *         ndl_s = normal . l_s
 *         if ndl_s > 0.0:
 *             den = p_L(position, l_s) + ndl_s * RR_FRAC_1_PI
 *             if den < +inf:                                      (false for NaN as well)
 *                 C = ((albedo * RR_FRAC_1_PI) * ndl_s) / den     (Div<f64> multiplies by the reciprocal)
 *                 hit_s = Bvh::intersect(Ray{position, l_s}, z_near, z_far)       one query, counted
 *                 if hit_s is Hit and its object is in the list:
 *                     light = light + (throughput * C) * hit_s.obj.emission.emit()
 *         l = ev.ray.direction;  ndl = normal . l;  pc = ndl * RR_FRAC_1_PI;  pl = p_L(position, l)
 *         w_next = pc / (pc + pl) if pl > 0.0 else 1.0            (a NaN pl: 1.0)
 *     else: w_next = 1.0
 *     throughput = throughput * ev.color;  the roulette and DivAssign as in the reference (one draw);  w = w_next;  r = ev.ray
 * The shadow sample is credited BEFORE the roulette: it is traced even if the roulette then ends the path, and at the last
 * bounce max_bounces allows.  The shadow query does not count against max_bounces; it does count in queries_i, which can
 * therefore reach S * (2 * max_bounces + 1).  A miss, and a listed object met by the first ray, are as in RADIANCE QUERY: w is 1
 * there.  The shadow query is the closest-hit query, whole; there is no any-hit shortcut.
 *
 * Why it is unbiased.  Seen from a diffuse point, a direction l has density p_L(l) under the light arm and pc(l) under the
 * cosine arm.  Light that a LISTED object sends along l is collected twice: by the shadow sample when the light arm draws l,
 * with weight p_L / (p_L + pc) -- C is brdf * cosine / p_L times that weight --, and by the continuation when the cosine arm
 * draws l and the next hit is listed, with weight w = pc / (p_L + pc).  The two weights sum to 1 wherever a listed object is the
 * first thing seen along l (where it is not, the shadow sample is blocked and p_L prices a light the continuation does not
 * meet: both sides collect nothing of it).  Objects outside the list keep their full weight and are found by BSDF sampling
 * alone, as is the environment.  A bounce that is not diffuse has no light arm, so what it meets next has weight 1.
 *
 * Which materials a listed emitter may have.  The reference adds a hit's emission only inside Scatter (lib.rs:530-550): an
 * emitter whose material can answer NoScatter radiates less than emit(), and the shadow sample, which credits emit() whole,
 * would over-credit it.  So a listed object with emission.emit() != 0 must have a material whose scatter has no NoScatter
 * path: LambertianDiffuse, Reflect or Glass (material.rs: Refract answers NoScatter at total internal reflection, the three
 * Cook-Torrance materials and Plastic's specular arm where a sampled direction is rejected or worth zero, NoReflect always).
 * Any other material on a listed emitter is RAYRS_UNSUPPORTED.  A dark listed object (a portal) may have any material.
 *
 * K = 0: every entry point below returns, bit for bit and count for count, what its unlit counterpart returns; no extra draw
 * is taken.
 *
 * RADIANCE, DIRECT (rayrs_scene_radiance_direct): RADIANCE QUERY with the turn above.
 * IRRADIANCE, DIRECT (rayrs_scene_irradiance_direct): with K >= 1 the point is a virtual Lambertian bounce of albedo (1, 1, 1)
 * at position = p_i + n_i * bias, normal n_i.  Draws 0 and 1 make IRRADIANCE's cosine ray l, exactly as in the unlit form; draws
 * 2, 3 and 4 are b, u1, u2; the shadow sample's credit is C * emit (throughput is 1); w for the first ray is w_next as above;
 * there is no roulette at the virtual bounce; and
 *     L_{i,s} = credit + radiance(scene, Ray{position, l}, max_bounces)     the path going on at draw 5.
 * max_bounces == 0: +0, 0 queries, no shadow query.
 * IMAGE FORM (rayrs_render_direct): pixels, keys, the primary ray, the sums and the fast_traversal treatment are
 * rayrs_render_lit's.  The sums, sample_chunk, index_base and seed are RADIANCE QUERY's throughout.
 *
 * `lights` is a HOST pointer in every form, as in LIGHT SAMPLING.  Refusals: LIGHT SAMPLING's, in its order, with the material
 * rule above in the RAYRS_UNSUPPORTED group (after the triangle check), and the overflow guard
 * (uint64)samples * (2 * max_bounces + 1) >= 2^32 in place of RADIANCE QUERY's. */
int rayrs_scene_radiance_direct(rayrs_scene* scene, const double* origin, const double* direction, uint64_t n, uint32_t samples,
                                uint32_t max_bounces, uint32_t sample_chunk, uint64_t seed, uint64_t index_base, uint32_t fast_traversal,
                                const uint32_t* lights, uint32_t n_lights, double* radiance /* may be NULL */,
                                uint32_t* queries /* may be NULL */);
int rayrs_scene_radiance_direct_launch(rayrs_scene* scene, const double* origin, const double* direction, uint64_t n, uint32_t samples,
                                       uint32_t max_bounces, uint32_t sample_chunk, uint64_t seed, uint64_t index_base,
                                       uint32_t fast_traversal, const uint32_t* lights, uint32_t n_lights,
                                       double* radiance /* may be NULL */, uint32_t* queries /* may be NULL */, void* hip_stream);
int rayrs_scene_irradiance_direct(rayrs_scene* scene, const double* position, const double* normal, uint64_t n, uint32_t samples,
                                  uint32_t max_bounces, uint32_t sample_chunk, double bias, uint64_t seed, uint64_t index_base,
                                  uint32_t fast_traversal, const uint32_t* lights, uint32_t n_lights,
                                  double* radiance /* may be NULL */, uint32_t* queries /* may be NULL */);
int rayrs_scene_irradiance_direct_launch(rayrs_scene* scene, const double* position, const double* normal, uint64_t n, uint32_t samples,
                                         uint32_t max_bounces, uint32_t sample_chunk, double bias, uint64_t seed, uint64_t index_base,
                                         uint32_t fast_traversal, const uint32_t* lights, uint32_t n_lights,
                                         double* radiance /* may be NULL */, uint32_t* queries /* may be NULL */, void* hip_stream);
int rayrs_render_direct(rayrs_scene* scene, const rayrs_camera* camera, uint64_t seed, uint32_t samples, uint32_t max_bounces,
                        uint32_t sample_chunk, uint32_t fast_traversal, const uint32_t* lights, uint32_t n_lights,
                        double* out_rgb /* H*W*3 */, uint32_t* queries /* H*W, may be NULL */);

/* ---- radiance queries with the sky among the lights: DIRECT LIGHTING above leaves the environment to BSDF sampling alone.  Here
 * the HDRI is one more light of it: directions are drawn from the map in proportion to its brightness, the same one shadow ray
 * per diffuse bounce may go to the sky, and the sky a continuation ray escapes to is weighted by the same balance heuristic.  A
 * map that is dark but for a window or a sun disc is to the environment what a small lamp is to the scene.  The reference clips
 * its map to [0, 3] (main.rs:42-43), so a texel is at most 3 and the gain is bounded by how uneven a clipped map can be.  The
 * kernels are a unit of their own (radiance_sky.hip); nothing above changes.
 *
 * SKY SAMPLING, specified to the operation.  Everything is f64 and unfused; the elementary functions are rayrs_numeric.h's.  w, h
 * are the HDRI's sizes; texel(i, j) is the clipped texel (row i, column j), widened to f64, that Scene::background reads.
 *
 * The table.  Built once per scene on the host from the host scene's HDRI (a scene made with device = -1 has one), lazily at the
 * first sky call, and uploaded once per device.  Its cells are the bilinear cells of background(): (i, j), i in 0..h-2, j in 0..w-2.
 *     L(i, j) = (r + g) + b of texel(i, j)
 *     s_i = rr_sin(((double)i + 0.5) * RR_PI / (double)(h - 1))
 *     A[i][j] = s_i * (((L(i,j) + L(i+1,j)) + L(i,j+1)) + L(i+1,j+1))
 *     C[i][j] = the inclusive prefix of A[i][.] in j order: the first assigned, then one add per cell
 *     R_i = C[i][w-2]
 *     M[i] = the inclusive prefix of R_. in i order, likewise
 *     T = M[h-2]
 * T not > 0.0, or not finite, is RAYRS_UNSUPPORTED: there is nothing to sample.  Additions of non-negative f64 are monotone, so
 * the prefixes are non-decreasing, and "the first index whose prefix exceeds the target" is the same index for any search.
 *
 * sky_sample(u1, u2):
 *     ty = u1 * T;  i = the first index with M[i] > ty, or h-2 if there is none
 *     below = i > 0 ? M[i-1] : 0.0;  y = (double)i + (ty - below) / R_i
 *     tx = u2 * R_i;  j = the first index with C[i][j] > tx, or w-2 if there is none
 *     below = j > 0 ? C[i][j-1] : 0.0;  x = (double)j + (tx - below) / A[i][j]
 *     theta = y / (double)(h - 1) * RR_PI;  phi = x / (double)(w - 1) * (2.0 * RR_PI);  psi = phi - RR_PI
 *     (st, ct) = rr_sincos(theta);  (sp, cp) = rr_sincos(psi);  l_s = (cp * st, ct, sp * st)
 * the inverse of background()'s mapping (lib.rs:254-285).  A 0 / 0 (a fall-through onto an empty row or cell) takes what IEEE
 * gives: the NaN direction then fails ndl_s > 0.0 and the sample is skipped.
 *
 * p_env(l):
 *     dir = l.unit();  phi, theta, x, y exactly Scene::background's (lib.rs:254-263)
 *     i = min(usize(floor(y)), h - 2);  j = min(usize(floor(x)), w - 2)
 *     sn = rr_sqrt(1.0 - dir.y * dir.y)
 *     p_env = ((A[i][j] / T) * ((double)(w - 1) * (double)(h - 1))) / (((2.0 * RR_PI) * RR_PI) * sn)
 * the solid-angle density of sky_sample's directions: A[i][j] / T of the draws fall in a cell, uniformly in (x, y), and a cell
 * spans 2 pi / (w - 1) of phi and pi / (h - 1) of theta.  At a pole sn = 0 and p_env = +inf: a shadow sample there is skipped
 * by den < +inf, and a continuation exactly along the axis gets weight 0 -- a set of measure zero.
 *
 * The turn is DIRECT LIGHTING's with M = K + 1 lights: K <= RAYRS_MAX_LIGHTS listed lamps, possibly none, and the sky, which is
 * index K.  What changes in it:
 *     b = rng.next();  u1 = rng.next();  u2 = rng.next()          the draws unchanged, always three
 *     k = min((uint32)(b * (double)M), M - 1);  l_s = sky_sample(u1, u2) if k == K, else light k's sample as in DIRECT LIGHTING
 *     p_M(position, l) = (p_0 assigned, then += p_k in list order, then += p_env(l) last; with K = 0, p_env assigned) / (double)M
 *         stands wherever DIRECT LIGHTING writes p_L(position, l): in den and in pm = p_M(position, ev.ray.direction)
 *     after hit_s = Bvh::intersect(Ray{position, l_s}, z_near, z_far), whichever k was drawn:
 *         if hit_s is Hit and its object is in the list:  light = light + (throughput * C) * hit_s.obj.emission.emit()
 *         if hit_s is Miss:  light = light + (throughput * C) * background(l_s)
 *     w_next = pc / (pc + pm) if pm > 0.0 else 1.0
 *     at a Miss of the path's own ray:  return light + throughput * (background(dir) * w)
 * w is 1.0 for a first ray and after a bounce that is not diffuse, so the background's bits are then the unlit ones.  Unlisted
 * objects keep weight 1.  The material rule for listed emitters, the overflow guard, queries_i (shadow rays counted),
 * IRRADIANCE's virtual bounce (draws 2, 3 and 4, the path going on at draw 5 -- here with K = 0 too, there is always the sky;
 * a virtual bounce's shadow ray that misses credits C * background(l_s)) and the image form are DIRECT LIGHTING's.
 *
 * Why it is unbiased.  Seen from a diffuse point, a direction l has density p_M(l) under the light arm and pc(l) under the cosine
 * arm.  Light arriving along l from the sky or from a listed object is collected by the shadow sample with weight
 * p_M / (p_M + pc) and by the continuation with weight pc / (p_M + pc): the two sum to 1 wherever the sky or a listed object is
 * the first thing seen along l.  Where p_M is 0 -- a black cell with no lamp behind it -- the light arm never draws l and the
 * continuation keeps weight 1.  Where an unlisted object is the first thing seen, the shadow sample is blocked and the
 * continuation meets an object of weight 1: both sides collect nothing of the light p_M prices.
 *
 * rayrs_scene_radiance_sky, rayrs_scene_irradiance_sky, their _launch forms and rayrs_render_sky take exactly the arguments of
 * their _direct counterparts: lights, n_lights name the lamps, the sky is always on, and n_lights == 0 is legal, the sky alone.
 * Every entry point above keeps its behaviour; the _direct calls still refuse the index 0xffffffff as an argument.  Refusals:
 * DIRECT LIGHTING's, in its order, with the empty table in the RAYRS_UNSUPPORTED group after the material rule.  The light
 * table stays in the kernel arguments and the sky's table is one device pointer beside it, so a _launch form allocates and
 * copies nothing after a scene's first sky call on a given walk.
 *
 * Three calls on the host, which need no device: the table's cells A in row order ((h-1)*(w-1) f64, may be NULL) and T;
 * sky_sample of n pairs (u1, u2); p_env of n directions.  The last two refuse an empty table as RAYRS_UNSUPPORTED. */
int rayrs_scene_radiance_sky(rayrs_scene* scene, const double* origin, const double* direction, uint64_t n, uint32_t samples,
                             uint32_t max_bounces, uint32_t sample_chunk, uint64_t seed, uint64_t index_base, uint32_t fast_traversal,
                             const uint32_t* lights, uint32_t n_lights, double* radiance /* may be NULL */,
                             uint32_t* queries /* may be NULL */);
int rayrs_scene_radiance_sky_launch(rayrs_scene* scene, const double* origin, const double* direction, uint64_t n, uint32_t samples,
                                    uint32_t max_bounces, uint32_t sample_chunk, uint64_t seed, uint64_t index_base,
                                    uint32_t fast_traversal, const uint32_t* lights, uint32_t n_lights,
                                    double* radiance /* may be NULL */, uint32_t* queries /* may be NULL */, void* hip_stream);
int rayrs_scene_irradiance_sky(rayrs_scene* scene, const double* position, const double* normal, uint64_t n, uint32_t samples,
                               uint32_t max_bounces, uint32_t sample_chunk, double bias, uint64_t seed, uint64_t index_base,
                               uint32_t fast_traversal, const uint32_t* lights, uint32_t n_lights,
                               double* radiance /* may be NULL */, uint32_t* queries /* may be NULL */);
int rayrs_scene_irradiance_sky_launch(rayrs_scene* scene, const double* position, const double* normal, uint64_t n, uint32_t samples,
                                      uint32_t max_bounces, uint32_t sample_chunk, double bias, uint64_t seed, uint64_t index_base,
                                      uint32_t fast_traversal, const uint32_t* lights, uint32_t n_lights,
                                      double* radiance /* may be NULL */, uint32_t* queries /* may be NULL */, void* hip_stream);
int rayrs_render_sky(rayrs_scene* scene, const rayrs_camera* camera, uint64_t seed, uint32_t samples, uint32_t max_bounces,
                     uint32_t sample_chunk, uint32_t fast_traversal, const uint32_t* lights, uint32_t n_lights,
                     double* out_rgb /* H*W*3 */, uint32_t* queries /* H*W, may be NULL */);
int rayrs_scene_sky_table(rayrs_scene* scene, double* cells /* (h-1)*(w-1), may be NULL */, double* total);
int rayrs_scene_sky_sample(rayrs_scene* scene, const double* u /* n*2 */, uint64_t n, double* dir /* n*3 */);
int rayrs_scene_sky_density(rayrs_scene* scene, const double* dir /* n*3 */, uint64_t n, double* p);

/* ---- radiance queries with a mesh-light group among the lights: DIRECT LIGHTING's lamps are spheres and axis-aligned rectangles,
 * at most RAYRS_MAX_LIGHTS of them, because every density there sums over the whole list.  A scene's lamp is as often a mesh: a
 * tube, a tilted panel, a glowing object.  Here any number of listed triangles together are ONE more light of DIRECT LIGHTING /
 * SKY SAMPLING: it is chosen like a lamp, its points are drawn uniformly by area from a prefix table in device memory, and it is
 * weighted by the balance heuristic in AREA measure at the first visible point, so no density ever sums over the list.  The
 * kernels are a unit of their own (radiance_mesh.hip); nothing above changes.
 *
 * MESH LIGHTS, specified to the operation.  Everything is f64 and unfused; the draws are taken from the path's rng in program
 * order; the elementary functions are rayrs_numeric.h's.
 *
 * The handle.  rayrs_mesh_lights_create makes a group of the n_tris triangles `tris` (a HOST array of object indices in the
 * numbering rayrs_scene_intersect returns; it is copied).  The handle is bound to its scene and must be destroyed before it.  It
 * owns the table on the host and its device copy, which is uploaded once, at the handle's first call that launches; a handle of
 * a host-only scene (device -1) serves the three host calls below.  n_tris == 0 is a legal, empty group.
 * rayrs_mesh_lights_destroy waits for the scene's radiance work that may still read the device copy, then frees it.  Refusals at
 * creation, in this order.  RAYRS_INVALID_ARG: a NULL scene or out; tris == NULL with n_tris > 0; an index >= the object count;
 * a duplicate index; n_tris >= 2^31.  RAYRS_UNSUPPORTED: an index that names a sphere or a plane; a listed triangle that emits
 * and whose material is not LambertianDiffuse, Reflect or Glass (DIRECT LIGHTING's material rule, unchanged: a dark triangle may
 * be anything); with n_tris >= 1, a total area T that is not > 0.0 or not finite.
 *
 * The table.  N = n_tris entries in list order.  For entry j, p1, p2, p3 are the host scene's f64 vertices and
 *     e1 = p2 - p1;  e2 = p3 - p1;  nrm = e1.cross(e2)            Triangle::new's own arithmetic (geometry.rs:341-353)
 *     n_j = nrm.unit();  A_j = nrm.mag() / 2.0                    (mag = rr_sqrt(nrm . nrm); unit multiplies by 1.0 / mag)
 *     P[j] = the inclusive prefix of A in list order: the first assigned, then one add per entry
 *     T = P[N-1]
 * Beside each entry the table keeps the slot the closest-hit walk reports for that triangle, and a bitmap over the scene's
 * primitive slots says which are listed.  A zero-area triangle is legal: the search below never lands on it unless it is the
 * fall-through entry, and there IEEE gives 0 / 0 -- the NaN direction fails ndl_s > 0.0, as SKY SAMPLING's empty cell does.
 *
 * mesh_sample(u1, u2):
 *     ty = u1 * T;  j = the first index with P[j] > ty, or N-1 if there is none
 *     below = j > 0 ? P[j-1] : 0.0;  r = (ty - below) / A_j
 *     su = rr_sqrt(r);  b0 = 1.0 - su;  b1 = su * (1.0 - u2);  b2 = su * u2
 *     q = (p1 * b0 + p2 * b1) + p3 * b2                           (per component)
 * u1 chooses the triangle and is rescaled for the point, as sky_sample rescales its row draw.
 *
 * p_tri(position, j, q):
 *     l_s = (q - position).unit()
 *     p_tri = (position - q).mag2() / (|n_j . l_s| * T)
 * the solid-angle density at `position` of mesh_sample's points AT q: 1 / T per area, times distance^2 / cosine.  It prices the
 * one point, not the direction: other listed triangles crossed by the same line are not in it.
 *
 * The turn is DIRECT LIGHTING's, or SKY SAMPLING's with sky = 1.  G = 1 if N >= 1, else 0; M = K + G + sky lights: the lamps are
 * indices 0 .. K-1, the group is K, the sky is last.  With G = 1 every diffuse bounce has the three draws, whatever K and sky are:
 *     b = rng.next();  u1 = rng.next();  u2 = rng.next()
 *     k = min((uint32)(b * (double)M), M - 1)
 *     p_R(position, l) = (the lamps' p_k in list order, the first assigned, then, with sky = 1, += p_env(l) last -- with K = 0,
 *         p_env assigned) / (double)M; with K = 0 and sky = 0 it is 0.0: the lamps' and the sky's density, the group's not in it
 *     if k == K (the group):
 *         (j, q) = mesh_sample(u1, u2);  l_s and p_tri as above;  ndl_s = normal . l_s
 *         if ndl_s > 0.0:
 *             den = p_tri / (double)M + ndl_s * RR_FRAC_1_PI
 *             if den < +inf:
 *                 C = ((albedo * RR_FRAC_1_PI) * ndl_s) / den
 *                 hit_s = Bvh::intersect(Ray{position, l_s}, z_near, z_far)       one query, counted
 *                 if hit_s is Hit and its object IS triangle j:  light = light + (throughput * C) * emit of that triangle
 *         anything else in front earns nothing: another listed triangle, a lamp, and a Miss even with the sky on
 *     else (a lamp, or the sky):
 *         l_s as in DIRECT LIGHTING / SKY SAMPLING;  den = p_R(position, l_s) + ndl_s * RR_FRAC_1_PI;  the rest unchanged:
 *         credited on a listed LAMP, or on a Miss with sky = 1; meeting a listed triangle earns nothing
 *     l = ev.ray.direction;  pc = (normal . l) * RR_FRAC_1_PI;  pr = p_R(position, l)
 *     w_next = pc / (pc + pr) if pr > 0.0 else 1.0                the weight of a listed lamp, or of the sky, met next
 *     the path keeps pc, and that its ray leaves a diffuse bounce
 * At the next hit, where ev scatters, with Ray{o, d} the path's ray, t the hit's and normal the hit's (Triangle::normal):
 *     if obj is a listed triangle:
 *         if the ray left a diffuse bounce:
 *             p = (o - ray.point(t)).mag2() / (|normal . d| * T)
 *             wt = pc / (pc + p / (double)M) if p > 0.0 else 1.0  (a NaN p: 1.0)
 *             e = emit * wt
 *         else e = emit                                           (a first ray, or a bounce that is not diffuse: weight 1)
 *     else if obj is a listed lamp: e = emit * w                  as before
 *     else e = emit                                               unlisted objects keep weight 1, emissive triangles outside
 *                                                                 the group included
 * A Miss of the path's own ray is SKY SAMPLING's (background * w) with sky = 1 and the unlit one with sky = 0.  IRRADIANCE's
 * virtual bounce is DIRECT LIGHTING's with this turn (draws 2, 3 and 4, the path going on at draw 5, its first ray leaving a
 * diffuse bounce); it is present whenever K + G + sky >= 1.  The overflow guard, the material rule for listed lamps,
 * queries_i (shadow rays counted), max_bounces == 0 and the image form are DIRECT LIGHTING's.
 *
 * Why it is unbiased.  Light leaving a first-visible point y of a listed triangle along l towards a diffuse point is collected
 * by two techniques only.  The group's arm, when it draws y: its solid-angle density there is p_tri / M -- drawing a point that
 * is hidden, by anything, earns nothing, so hidden crossings of the same line do not count.  And the continuation, when the
 * cosine arm draws l: density pc.  The two weights are p / (p + pc) with p = p_tri / M -- C is brdf * cosine / p times that --
 * and pc / (p + pc), both evaluated at that same point, and they sum to 1 up to the rounding between q and the hit point.  Lamp-
 * and sky-drawn samples never collect a triangle and group-drawn samples never collect a lamp or the sky, so DIRECT LIGHTING's
 * and SKY SAMPLING's argument stands as written for the lamps and the sky, with the new M in their arm's probability.
 *
 * When the group is empty (mesh == NULL, or a handle of no triangles): G = 0, and the entry points below return, bit for bit and
 * count for count, what their _direct counterparts return with sky = 0 and what their _sky counterparts return with sky = 1 --
 * and therefore the unlit answers with K = 0 and no sky.
 *
 * rayrs_scene_radiance_mesh, rayrs_scene_irradiance_mesh, their _launch forms and rayrs_render_mesh take the arguments of their
 * _direct counterparts plus the group and sky (0 or 1).  Refusals: DIRECT LIGHTING's in its order (SKY SAMPLING's with sky = 1);
 * a handle of another scene, and a sky above 1, join the RAYRS_INVALID_ARG group; RAYRS_NO_DEVICE comes last.  The lamps stay in
 * the kernel arguments and the group is two device pointers and T beside them, so a _launch form allocates and copies nothing
 * after a handle's first device call on a given walk.  All twenty-four path kernels of the unit (both record formats, both
 * walks, without and with the sky, the three starts) use at most 256 VGPRs, no scratch and no static LDS.
 *
 * Three calls on the host, which need no device: the areas A_j in list order (N f64, may be NULL) and T; mesh_sample of n pairs
 * (u1, u2) -> j and q; p_tri of n (position, j, q).  The last two refuse an empty group as RAYRS_UNSUPPORTED, and the last a j
 * that is not below N as RAYRS_INVALID_ARG. */
typedef struct rayrs_mesh_lights rayrs_mesh_lights;
int rayrs_mesh_lights_create(rayrs_scene* scene, const uint32_t* tris, uint64_t n_tris, rayrs_mesh_lights** out);
void rayrs_mesh_lights_destroy(rayrs_mesh_lights* mesh);
int rayrs_mesh_lights_table(const rayrs_mesh_lights* mesh, double* areas /* N, may be NULL */, double* total);
int rayrs_mesh_lights_sample(const rayrs_mesh_lights* mesh, const double* u /* n*2 */, uint64_t n, uint32_t* j /* n */,
                             double* q /* n*3 */);
int rayrs_mesh_lights_density(const rayrs_mesh_lights* mesh, const double* position /* n*3 */, const uint32_t* j /* n */,
                              const double* q /* n*3 */, uint64_t n, double* p);
int rayrs_scene_radiance_mesh(rayrs_scene* scene, const double* origin, const double* direction, uint64_t n, uint32_t samples,
                              uint32_t max_bounces, uint32_t sample_chunk, uint64_t seed, uint64_t index_base, uint32_t fast_traversal,
                              const uint32_t* lights, uint32_t n_lights, const rayrs_mesh_lights* mesh /* may be NULL: empty */,
                              uint32_t sky, double* radiance /* may be NULL */, uint32_t* queries /* may be NULL */);
int rayrs_scene_radiance_mesh_launch(rayrs_scene* scene, const double* origin, const double* direction, uint64_t n, uint32_t samples,
                                     uint32_t max_bounces, uint32_t sample_chunk, uint64_t seed, uint64_t index_base,
                                     uint32_t fast_traversal, const uint32_t* lights, uint32_t n_lights,
                                     const rayrs_mesh_lights* mesh /* may be NULL: empty */, uint32_t sky,
                                     double* radiance /* may be NULL */, uint32_t* queries /* may be NULL */, void* hip_stream);
int rayrs_scene_irradiance_mesh(rayrs_scene* scene, const double* position, const double* normal, uint64_t n, uint32_t samples,
                                uint32_t max_bounces, uint32_t sample_chunk, double bias, uint64_t seed, uint64_t index_base,
                                uint32_t fast_traversal, const uint32_t* lights, uint32_t n_lights,
                                const rayrs_mesh_lights* mesh /* may be NULL: empty */, uint32_t sky,
                                double* radiance /* may be NULL */, uint32_t* queries /* may be NULL */);
int rayrs_scene_irradiance_mesh_launch(rayrs_scene* scene, const double* position, const double* normal, uint64_t n, uint32_t samples,
                                       uint32_t max_bounces, uint32_t sample_chunk, double bias, uint64_t seed, uint64_t index_base,
                                       uint32_t fast_traversal, const uint32_t* lights, uint32_t n_lights,
                                       const rayrs_mesh_lights* mesh /* may be NULL: empty */, uint32_t sky,
                                       double* radiance /* may be NULL */, uint32_t* queries /* may be NULL */, void* hip_stream);
int rayrs_render_mesh(rayrs_scene* scene, const rayrs_camera* camera, uint64_t seed, uint32_t samples, uint32_t max_bounces,
                      uint32_t sample_chunk, uint32_t fast_traversal, const uint32_t* lights, uint32_t n_lights,
                      const rayrs_mesh_lights* mesh /* may be NULL: empty */, uint32_t sky, double* out_rgb /* H*W*3 */,
                      uint32_t* queries /* H*W, may be NULL */);

/* ------------------------------------------------------------------------------------------------------------------
 * DIRECT-LIT FILMS.  A film whose passes are direct-lit: rayrs_film_create_direct makes a film of DIRECT LIGHTING's paths,
 * rayrs_film_create_sky one of SKY SAMPLING's (lights, n_lights name the lamps, the sky is always on, n_lights == 0 is legal: the
 * sky alone).  lights is a HOST array, copied at creation and fixed for the film's life.  The film is a rayrs_film like any
 * other: every rayrs_film_* call and rayrs_history_push_film takes it.
 *
 * THE CONTRACT and THE CONTRACT PER TILE of the progressive film hold word for word with rayrs_render_direct (rayrs_render_sky)
 * in rayrs_render's place, called with the same seed, max_bounces, sample_chunk = c, list, and the walk a render with the film's
 * settings takes: after passes adding up to N_t samples in tile t, rayrs_film_read(RAYRS_OUT_F64) returns, bit for bit, that
 * entry point's pixels for samples = N_t; RAYRS_OUT_F32 is that value converted; a film with tile_ranks > 1 holds its share's
 * pixels and the rest read +0.  No arithmetic differs: the first chunk sum is assigned, later ones are added in chunk order, then
 * sum * (1.0 / N), in the image form's resolve as in the film's records.  A film with an empty list (rayrs_film_create_direct,
 * n_lights == 0) holds a plain film's records.  NOISE, ADAPTIVE PASSES, NOISE PLANE, FEATURES, DENOISER, GUIDED FILTER and
 * TEMPORAL ACCUMULATION apply unchanged: they read the records and the first-hit features only.
 *
 * rayrs_film_status.rays is the closest-hit queries the film's paths made, shadow rays included: the sum over the share's
 * in-image pixels of the `queries` plane rayrs_render_direct (rayrs_render_sky) returns at N_t; paths is the in-image pixels of
 * the sampled tiles times n, summed over the passes.  pass_stats carries the pass's rays and paths, exact_walk as chosen, and
 * one HIP-event time of all the pass's kernels in kernel_ms and total_ms; every field that describes the path pool, its rounds
 * or the work counters is 0.
 *
 * Refusals at creation, before the device is touched.  RAYRS_INVALID_ARG: rayrs_film_create's of that group; lights == NULL with
 * n_lights > 0; an index >= the scene's object count.  Then RAYRS_UNSUPPORTED: rayrs_film_create's of that group;
 * n_lights > RAYRS_MAX_LIGHTS; an index naming a triangle; DIRECT LIGHTING's material rule; for rayrs_film_create_sky the empty
 * table; c * (2 * max_bounces + 1) >= 2^32 (an item's query counter is 32 bits).  Then RAYRS_NO_DEVICE.
 *
 * A pass: a tile's items of one pass fit one launch of the waves, ceil(n / c) * 64 <= 2^20, that is n / c up to 16384; a longer
 * pass is RAYRS_UNSUPPORTED and leaves the film unchanged.  The other pass rules are the progressive film's (n = 0, a closed
 * film, the 2^30 sample cursor, an adaptive pass's n % c).
 *
 * The checkpoint image is the progressive film's, byte for byte the same format: the light list is NOT recorded in it, just as
 * the scene and the camera are not.  Continuing a direct-lit film's image on a film with another list, or on a plain film (or a
 * plain film's image on a direct-lit film), is the caller's error: rayrs_film_state_set cannot tell, and the result is the mean
 * of samples of different estimators. */
int rayrs_film_create_direct(rayrs_scene* scene, const rayrs_camera* camera, const rayrs_film_params* params,
                             const uint32_t* lights /* HOST */, uint32_t n_lights, rayrs_film** out);
int rayrs_film_create_sky(rayrs_scene* scene, const rayrs_camera* camera, const rayrs_film_params* params,
                          const uint32_t* lights /* HOST */, uint32_t n_lights, rayrs_film** out);

/* ------------------------------------------------------------------------------------------------------------------
 * BAKE.  The progressive film's machinery for the callers of the radiance queries: a bake is a device-resident accumulation
 * buffer over n rays or points of the caller's -- lightmap texels, probe positions -- bound to one scene, one strategy (unlit,
 * DIRECT LIGHTING, SKY SAMPLING) and one set of sampling settings, to which samples are added in passes, to every point or only
 * to the points the noise estimate calls for.  Points are independent, so the unit of everything below is the single point i
 * with its own sample count N_i.  a and b are HOST arrays of n*3 f64 (kind 0: positions and normals, kind 1: origins and
 * directions), copied to the device at creation; lights is a HOST array, copied at creation and fixed for the bake's life.
 *
 * THE CONTRACT PER POINT.  After any sequence of passes that leaves point i at N_i samples, rayrs_bake_read returns for point i,
 * bit for bit, the radiance the matching query returns for that one point with samples = N_i, sample_chunk = c,
 * index_base = index_base + i and the same seed, max_bounces, bias, walk and list, and as its query count that call's `queries`,
 * kept in 64 bits.  The matching query: kind 0 rayrs_scene_irradiance (sky = 0, n_lights == 0), rayrs_scene_irradiance_direct
 * (sky = 0, n_lights > 0) or rayrs_scene_irradiance_sky (sky = 1); kind 1 the _radiance ones.  (A bake with sky = 0 and an empty
 * list runs DIRECT LIGHTING's paths with K = 0, which are the unlit query's bit for bit.)  This holds for every partition into
 * passes that the rules allow and across a rayrs_bake_state_get / new bake / rayrs_bake_state_set in between: a sample's random
 * numbers depend on (seed, index_base + i, sample index) only, the record's sum starts by assignment with the first chunk sum,
 * later chunk sums are added in chunk order, and the read is sum * (1.0 / N_i).  A point without samples reads +0 and 0.
 *
 * RULES.  The progressive film's, per point.  c = sample_chunk is fixed for the bake's life; while the bake is open every N_i is
 * a multiple of c.  rayrs_bake_render(n) adds the samples N_i .. N_i + n - 1 to every point from its own N_i, and CLOSES the bake
 * if n % c != 0; n = 0, or any pass on a closed bake, is RAYRS_INVALID_ARG and changes nothing.  (largest N_i) + n < 2^30, else
 * RAYRS_UNSUPPORTED.  A pass of more than 2^16 chunks per point (ceil(n / c) > 65536) is RAYRS_UNSUPPORTED and leaves the bake
 * unchanged.  An adaptive pass needs n % c == 0 (else RAYRS_INVALID_ARG) and never closes the bake.  A pass uses the scene's
 * radiance scratch and stack strip under the queries' ordering rule, and is synchronous.  max_bounces == 0: every sample is +0 and
 * makes no query, as the queries have it.  The scene outlives its bakes; the calls on one scene, its films and its bakes come from
 * one thread at a time.
 *
 * NOISE is the film's, word for word, with M_i = N_i / c per point: S1 and S2 are the sums over the point's full chunks of
 * y = (x + y) + z of the chunk sum and of y*y, accumulated in chunk order starting by assignment, unfused; the converged-at-tau
 * predicate and the non-finite rule are NOISE's.  rayrs_bake_noise is NOISE PLANE's formula per point with M = M_i: +infinity
 * for M_i < 2 or non-finite sums, selected and never computed.
 *
 * SELECTION.  rayrs_bake_render_adaptive(n, tau, max_point_samples) takes point i iff N_i + n <= max_point_samples (0 = no cap
 * but the 30-bit cursor) and the point is unconverged at tau; a non-finite point is never taken.  The selected points are sampled
 * in ascending index order, so a pass's work is a function of the bake's state alone.  *active_points = the number selected; 0
 * is RAYRS_OK with no launch and stats zeroed.  tau: finite and >= 0.
 *
 * rayrs_bake_pass: points = the points the pass sampled, paths = points * n, rays = the closest-hit queries its paths made
 * (shadow rays included), kernel_ms = one HIP-event time of all the pass's kernels, total_ms = the call's wall time, launches =
 * the launches of the wave kernels.  rayrs_bake_status: samples = the largest N_i, rays and paths summed over all passes,
 * unconverged and nonfinite by NOISE at the call's tau, points = n.
 *
 * Refusals at creation, all decided before the device is touched, in the queries' order.  RAYRS_INVALID_ARG: a NULL scene, a, b,
 * params or out; fast_traversal > 1; kind > 1; sky > 1; pad != 0; lights == NULL with n_lights > 0; an index >= the scene's
 * object count.  Then RAYRS_UNSUPPORTED: c >= 2^30; max_bounces > 8000; c * max_bounces >= 2^32 for the unlit bake,
 * c * (2 * max_bounces + 1) >= 2^32 for the others (an item's query counter is 32 bits); n_lights > RAYRS_MAX_LIGHTS; an index
 * naming a triangle; DIRECT LIGHTING's material rule; with sky = 1 the empty table; n >= 2^32.  Then RAYRS_NO_DEVICE.  n == 0 on
 * a device scene makes a legal, empty bake: its passes launch nothing and its reads return nothing.
 *
 * Checkpoint: an opaque, versioned byte image -- the records, the query counts, the sample counts, the counters and the settings
 * (kind, sky, c, max_bounces, walk, seed, index_base, bias) and n.  The points, the scene and the list are NOT recorded, as a
 * film's camera and list are not: continuing on other points is the caller's error.  rayrs_bake_state_set refuses
 * (RAYRS_INVALID_ARG, the bake unchanged) an image of another image version, settings or n, or a length that is not
 * rayrs_bake_state_bytes.  The footprint on the device: 100 bytes per point (48 of them the point itself). */
typedef struct rayrs_bake rayrs_bake;

typedef struct {            /* zero-initialise */
    uint32_t kind;          /* 0: irradiance (a = positions, b = normals); 1: radiance (a = origins, b = directions) */
    uint32_t sample_chunk;  /* c >= 1, fixed for the bake's life; 0 = 4 */
    uint32_t max_bounces;
    uint32_t fast_traversal;/* taken as asked, as the queries take it */
    uint64_t seed, index_base;
    double   bias;          /* kind 0 only */
    uint32_t sky;           /* 1: SKY SAMPLING's paths (lights may be empty); 0: DIRECT LIGHTING's, the unlit ones with n_lights == 0 */
    uint32_t pad;
} rayrs_bake_params;

typedef struct {
    uint64_t points;        /* the points the pass sampled */
    uint64_t paths, rays;
    double kernel_ms, total_ms;
    uint32_t launches, pad;
} rayrs_bake_pass;

typedef struct {
    uint64_t samples;       /* the largest N_i */
    uint64_t rays, paths;   /* summed over all passes */
    uint64_t unconverged, nonfinite; /* NOISE, for the tau of the call */
    uint64_t points;        /* n */
    uint32_t closed;        /* 1 = the last pass ended in a short chunk: no further pass is accepted */
    uint32_t pad;
} rayrs_bake_status;

int rayrs_bake_create(rayrs_scene* scene, const double* a, const double* b, uint64_t n, const rayrs_bake_params* params,
                      const uint32_t* lights /* HOST */, uint32_t n_lights, rayrs_bake** out);
void rayrs_bake_destroy(rayrs_bake* bake);
int rayrs_bake_render(rayrs_bake* bake, uint32_t n_samples, rayrs_bake_pass* stats /* may be NULL */);
int rayrs_bake_render_adaptive(rayrs_bake* bake, uint32_t n_samples, double tau, uint32_t max_point_samples,
                               uint64_t* active_points /* may be NULL */, rayrs_bake_pass* stats /* may be NULL */);
/* host buffers; either may be NULL = not wanted, not both */
int rayrs_bake_read(rayrs_bake* bake, double* radiance /* n*3 */, uint64_t* queries /* n */);
int rayrs_bake_point_samples(rayrs_bake* bake, uint32_t* out /* n */);
int rayrs_bake_noise(rayrs_bake* bake, double* variance /* n */);
int rayrs_bake_status_get(rayrs_bake* bake, double tau, rayrs_bake_status* out);
uint64_t rayrs_bake_state_bytes(const rayrs_bake* bake);
int rayrs_bake_state_get(rayrs_bake* bake, void* out_host, uint64_t cap);
int rayrs_bake_state_set(rayrs_bake* bake, const void* in_host, uint64_t bytes);

/* ------------------------------------------------------------------------------------------------------------------
 * MESH-LIT FILMS AND BAKES.  MESH LIGHTS' group in the two accumulating forms: rayrs_film_create_mesh makes a film, and
 * rayrs_bake_create_mesh a bake, whose passes run MESH LIGHTS' paths -- the lamps of `lights`, the group, and the sky with
 * sky = 1 (the bake: params->sky = 1).  lights is a HOST array, copied at creation; n_lights == 0 is legal (the group alone, or
 * with the sky).  The film is a rayrs_film and the bake a rayrs_bake like any other: every rayrs_film_* call,
 * rayrs_history_push_film and every rayrs_bake_* call take them unchanged.  The kernels are two units of their own
 * (film_mesh.hip, bake_mesh.hip): MESH LIGHTS' wave, started as DIRECT-LIT FILMS and BAKE start theirs; nothing above changes.
 *
 * THE FILM.  DIRECT-LIT FILMS' contract holds word for word with rayrs_render_mesh in rayrs_render_direct's place: after passes
 * adding up to N_t samples in tile t, rayrs_film_read(RAYRS_OUT_F64) returns, bit for bit, rayrs_render_mesh's pixels for
 * samples = N_t, called with the same seed, max_bounces, sample_chunk = c, list, group, sky and the walk a render with the
 * film's settings takes; RAYRS_OUT_F32 is that value converted; a film with tile_ranks > 1 holds its share's pixels and the rest
 * read +0.  This holds for every partition into passes the rules allow, uniform or adaptive, and across a rayrs_film_state_get /
 * new film / rayrs_film_state_set in between.  rayrs_film_status.rays is the sum over the share's in-image pixels of the
 * `queries` plane rayrs_render_mesh returns at N_t, shadow rays included; paths and pass_stats are DIRECT-LIT FILMS'.  The pass
 * rules are DIRECT-LIT FILMS', the limit of 16384 chunks per pass among them (a longer pass is RAYRS_UNSUPPORTED and leaves the
 * film unchanged).  NOISE, ADAPTIVE PASSES, NOISE PLANE, FEATURES, DENOISER, GUIDED FILTER and TEMPORAL ACCUMULATION apply
 * unchanged.
 *
 * THE BAKE.  BAKE's CONTRACT PER POINT holds with rayrs_scene_irradiance_mesh (kind 0) or rayrs_scene_radiance_mesh (kind 1) as
 * the matching query, called with the group and sky = params->sky on the one point with index_base = index_base + i.  RULES,
 * NOISE, SELECTION, rayrs_bake_pass and rayrs_bake_status are BAKE's, unchanged.
 *
 * THE EMPTY GROUP (mesh == NULL, or a handle of no triangles).  The film holds, byte for byte in rayrs_film_state_get, the
 * records of rayrs_film_create_direct's film (sky = 0) or rayrs_film_create_sky's (sky = 1) with the same list, and the bake
 * those of rayrs_bake_create's: their passes launch the direct and the sky kernels, as the queries' calls with an empty group do.
 *
 * Refusals at creation, all decided before the device is touched, in MESH LIGHTS' order: the film's are
 * rayrs_film_create_direct's in their order (sky = 1: rayrs_film_create_sky's), the bake's are rayrs_bake_create's in theirs; a
 * handle of another scene and, for the film, a sky above 1 join the RAYRS_INVALID_ARG group (the bake's sky is params->sky,
 * which BAKE refuses above 1 already); RAYRS_NO_DEVICE comes last.  A bake with a group of N >= 1 triangles is never the unlit
 * bake: its counter rule is c * (2 * max_bounces + 1) >= 2^32.
 *
 * Lifetime.  The film or the bake BORROWS the group: the handle must outlive every film and bake made with it, as the scene
 * outlives them, and is destroyed before the scene.  Its device table is uploaded at the first pass if no call has uploaded it
 * yet.  A pass runs under the queries' scratch ordering rule, so rayrs_mesh_lights_destroy's wait covers the last pass.
 *
 * Checkpoints.  Both images are byte for byte the formats they were: the group is NOT recorded, as the list is not.  Continuing an
 * image on a film or a bake with another group (or with none) is the caller's error, which rayrs_film_state_set and
 * rayrs_bake_state_set cannot tell: the result is the mean of samples of different estimators. */
int rayrs_film_create_mesh(rayrs_scene* scene, const rayrs_camera* camera, const rayrs_film_params* params,
                           const uint32_t* lights /* HOST */, uint32_t n_lights,
                           const rayrs_mesh_lights* mesh /* may be NULL: empty */, uint32_t sky, rayrs_film** out);
int rayrs_bake_create_mesh(rayrs_scene* scene, const double* a, const double* b, uint64_t n, const rayrs_bake_params* params,
                           const uint32_t* lights /* HOST */, uint32_t n_lights,
                           const rayrs_mesh_lights* mesh /* may be NULL: empty */, rayrs_bake** out);   /* sky: params->sky */

/* ------------------------------------------------------------------------------------------------------------------
 * LIGHT TREE.  MESH LIGHTS draws the group's points uniformly by area, from one table, for every shading point of the scene: a
 * point below one of sixty-four lamps aims 63 of 64 shadow rays at the others, and a large dim panel takes the draws a small
 * bright one beside it should have.  rayrs_mesh_lights_create_tree makes a group whose triangle is chosen, per shading point, by
 * the descent of a binary tree over the listed triangles, each branch in proportion to power over squared distance (Conty and
 * Kulla 2018, without the orientation cone: emitters here are two-sided).  MESH LIGHTS' weights are in area measure and never sum
 * over the list, so the one factor that changes is 1 / T, which becomes p_sel(j | x) / A_j.  The kernels are a unit of their own
 * (radiance_tree.hip); nothing above changes.
 *
 * LIGHT TREE, specified to the operation.  Everything is f64 and unfused; the elementary functions are rayrs_numeric.h's.
 *
 * The handle is a rayrs_mesh_lights: rayrs_mesh_lights_destroy, rayrs_mesh_lights_table, the binding to one scene and the lazy
 * device copy are MESH LIGHTS'.  Refusals at creation are rayrs_mesh_lights_create's, in its order, and RAYRS_UNSUPPORTED gains: a
 * listed triangle with a negative or non-finite emission channel; a non-finite vertex; with n_tris >= 1, a total power (the
 * root's W) that is not > 0.0 or not finite.  n_tris == 0 is a legal, empty group.
 *
 * Entries, in list order: p1, p2, p3, n_j, A_j and the slot are MESH LIGHTS'.  With e the emission of the triangle's surface,
 *     w_j = A_j * ((e_r + e_g) + e_b)                              the power of entry j
 * Dark and zero-area triangles are legal; an entry with w_j == 0 is never drawn (below).
 *
 * The build is deterministic and top-down over a permutation of the entries.  c = (p1 + p2) + p3 (per component, no division)
 * is an entry's centroid key.  A node over n > 1 entries takes lo and hi of its entries' keys per axis, picks the axis of the
 * largest hi - lo (a tie: the lowest axis), orders its entries by (c[axis], list index), gives the first ceil(n / 2) to its
 * left child and the rest to its right.  A node over one entry is a leaf.  Nodes are numbered in preorder: the root is 0, the
 * left child of node i is i + 1, the right child's index is kept; there are 2N - 1.  Each node keeps, with lo and hi now the box
 * over its entries' VERTICES (the first vertex assigned, then v < lo and v > hi compared),
 *     m = (lo + hi) * 0.5;  r2 = (hi - m).mag2();  W = W_left + W_right (a leaf: w_j)
 * and each entry its leaf's depth and its path word: bit k is set where the way from the root goes right at depth k.  The depth
 * is at most ceil(log2 N), below 32.
 *
 * One step at a node with children l and r, seen from x, with the draw u and the probability p so far:
 *     I_c = W_c > 0.0 ? W_c / rr_max(|x - m_c|^2, r2_c) : 0.0      (c = l, r; |.|^2 is mag2; rr_max ignores a NaN)
 *     s = I_l + I_r
 *     P_l = I_l / s if s > 0.0 && s < +inf, else W_l / (W_l + W_r)
 *     P_r = 1.0 - P_l
 *     left iff u < P_l:  u = u / P_l;  p = p * P_l                 else right:  u = (u - P_l) / P_r;  p = p * P_r
 *
 * tree_sample(x, u1, u2): descend from the root with u = u1, p = 1.0.  At the leaf of entry j:
 *     r = rr_min(u, 1.0)
 *     su = rr_sqrt(r);  b0, b1, b2 and q as mesh_sample has them from (r, u2)
 *     (j, q, p_sel = p)
 * tree_probability(x, j): the same descent, steered by j's path word instead of by u -- the same expressions in the same order,
 * so it returns, bit for bit, the p tree_sample returned when it arrived at j.
 *
 * The descent ends at a leaf within the table for ANY f64 x, u1 and u2, NaN and infinities included: a step never computes
 * where it goes, it follows one of the two child references the build wrote, so after at most depth steps it stands at a leaf,
 * whatever P_l is.  u < P_l is false when either side is NaN: a NaN comparison goes RIGHT.  A NaN or infinite |x - m|^2 gives
 * r2's importance or 0.0, an s that is not positive and finite gives the powers' ratio, and where that is 0 / 0 the step goes
 * right with a NaN p: the sample then fails den < +inf and casts no ray.  An entry with w_j == 0 is arrived at only with
 * p_sel == 0.0 or NaN (its side's P is 0.0 for every x), and such a sample earns nothing: a dark triangle's emission is 0 and a
 * zero-area one's p_tri is NaN.
 *
 * The turn is MESH LIGHTS', word for word, with two substitutions.  The group's arm:
 *     (j, q, p_sel) = tree_sample(position, u1, u2);  l_s = (q - position).unit()
 *     p_tri = ((position - q).mag2() / (|n_j . l_s| * A_j)) * p_sel
 * and a listed triangle met by a ray that left a diffuse bounce, with j the entry of the hit slot and o the ray's origin:
 *     p = ((o - ray.point(t)).mag2() / (|normal . d| * A_j)) * tree_probability(o, j)
 *     wt = pc / (pc + p / (double)M) if p > 0.0 else 1.0
 * The draws b, u1, u2 and their order, M, the lamps, the sky, p_R, "only the very triangle it drew earns", the query counts,
 * IRRADIANCE's virtual bounce and the image form are unchanged.  An empty tree group gives DIRECT LIGHTING's or SKY SAMPLING's
 * bits, as an empty group does.
 *
 * Why it is unbiased.  MESH LIGHTS' argument stands with one density replaced.  The group's arm arrives at a first-visible point
 * y of entry j with area density p_sel(j | x) / A_j -- the descent's probabilities of one node sum to 1 (P_r = 1.0 - P_l), so
 * the leaves' sum to 1 for the fixed x, and every entry that emits has p_sel > 0: a child with W > 0 has I > 0, or the powers'
 * ratio > 0 -- times distance^2 / cosine: p_tri, over M.  The continuation that meets y from o evaluates the same density, at the
 * same x = o, with tree_probability(o, j) = that p_sel bit for bit.  The two weights p / (p + pc) and pc / (p + pc) are taken at
 * the same point and sum to 1 up to the rounding between q and the hit point.  The position enters the DENSITY only, never the
 * set of points that can be drawn, so nothing that emits is left out.
 *
 * On the device the tree is one 128-byte line per interior node, holding both children's m, r2, W and where they are, so a step
 * reads one line; the record read at the leaf is MESH LIGHTS' 128-byte one with the path word, the depth and w_j in its padding;
 * and one u32 per primitive slot (the entry, or 0xFFFFFFFF) replaces the bitmap, so one load at a hit tells "listed?" and "which
 * entry".  rayrs_scene_radiance_mesh, rayrs_scene_irradiance_mesh, their _launch forms and rayrs_render_mesh take a tree handle
 * as `mesh` and tell it by its kind; their refusals are unchanged, and a _launch form still allocates and copies nothing after
 * the handle's first device call.  All twenty-four path kernels of the unit (both record formats, both walks, without and with
 * the sky, the three starts) use at most 256 VGPRs (209 to 228 as compiled), no scratch and no static LDS.
 *
 * rayrs_film_create_mesh and rayrs_bake_create_mesh REFUSE a tree handle, empty or not, as RAYRS_UNSUPPORTED, first of that
 * group and before the device is touched: their passes have no kernel that descends a tree, and they must not sample uniformly
 * in its place.
 *
 * Host calls, which need no device.  rayrs_mesh_lights_tree_nodes: the 2N - 1 nodes in preorder -- m, r2, W (five f64 each), the
 * right child's index (0xFFFFFFFF at a leaf) and the leaf's entry (0xFFFFFFFF at an interior node); any of the three may be
 * NULL, not all.  rayrs_mesh_lights_tree_entries: w_j, the path word and the depth of every entry, likewise.
 * rayrs_mesh_lights_tree_sample: tree_sample of n (position, u1, u2) -> j, q, p_sel.  rayrs_mesh_lights_tree_probability:
 * tree_probability of n (position, j).  rayrs_mesh_lights_density on a tree handle returns this section's p_tri of n
 * (position, j, q).  All four refuse a handle that is no tree as RAYRS_UNSUPPORTED, the last three an empty group as well, and a
 * j that is not below N is RAYRS_INVALID_ARG.  rayrs_mesh_lights_sample needs no position: on a tree handle it is
 * RAYRS_UNSUPPORTED. */
int rayrs_mesh_lights_create_tree(rayrs_scene* scene, const uint32_t* tris, uint64_t n_tris, rayrs_mesh_lights** out);
int rayrs_mesh_lights_tree_nodes(const rayrs_mesh_lights* mesh, double* mrw /* (2N-1)*5, may be NULL */,
                                 uint32_t* right /* 2N-1, may be NULL */, uint32_t* entry /* 2N-1, may be NULL */);
int rayrs_mesh_lights_tree_entries(const rayrs_mesh_lights* mesh, double* power /* N, may be NULL */, uint32_t* path /* N, may be NULL */,
                                   uint32_t* depth /* N, may be NULL */);
int rayrs_mesh_lights_tree_sample(const rayrs_mesh_lights* mesh, const double* position /* n*3 */, const double* u /* n*2 */,
                                  uint64_t n, uint32_t* j /* n */, double* q /* n*3 */, double* p_sel /* n */);
int rayrs_mesh_lights_tree_probability(const rayrs_mesh_lights* mesh, const double* position /* n*3 */, const uint32_t* j /* n */,
                                       uint64_t n, double* p /* n */);

/* SH PROBES.  The radiance that arrives at a point from every direction, projected onto the nine real spherical harmonics of
 * orders 0 to 2, per colour channel: the form an engine stores a light probe in.  A probe is a point x_i and nothing else; its
 * directions come from the library's counter RNG, so a result is a function of (seed, index_base + i) and a call on a slice of
 * the points with index_base moved is the slice of the whole call.  One pair of entry points serves every lighting of the
 * radiance queries: unlit, DIRECT LIGHTING's lamps, SKY SAMPLING's sky, MESH LIGHTS' group and LIGHT TREE's.
 *
 * SH PROBES, specified to the operation.  Everything is f64 and unfused; the elementary functions are rayrs_numeric.h's.  For
 * probe i at x_i (any f64 is legal) and sample s of S:
 *
 *     key = rr_path_key(seed, index_base + i, s)                        RADIANCE QUERY's key
 *     u1 = draw 0, u2 = draw 1                                           the direction: Sphere::sample (geometry.rs:142-152) on
 *     phi = 2.0 * RR_PI * u2;  (sn, cs) = rr_sincos(phi)                 the unit sphere at the origin -- LIGHT SAMPLING's sphere
 *     r = rr_sqrt(u1 * (1.0 - u1))                                       arm without the radius and the centre
 *     w = ((cs * 2.0) * r, (sn * 2.0) * r, 1.0 - 2.0 * u1)               used as given, NOT normalised again
 *     L_s = the lighting's path value along the ray (x_i, w), its rng going on at draw 2
 *
 * A probe is not a surface: there is no virtual bounce at the point (that is IRRADIANCE's).  Without lights, sky and group the
 * path is RADIANCE QUERY's; with any of them it is RADIANCE QUERY's path of DIRECT LIGHTING, SKY SAMPLING, MESH LIGHTS or LIGHT
 * TREE from its first hit on, w = 1.0 for the first ray.
 *
 * The basis, in the order (l, m) = (0,0), (1,-1), (1,0), (1,1), (2,-2), (2,-1), (2,0), (2,1), (2,2), on the components (x, y, z)
 * of w as they stand -- which axis is "up" is the caller's business: the library rotates nothing, z is the polar axis of these
 * formulas and of nothing else --, every product taken from left to right as bracketed:
 *
 *     Y_0 = K0          Y_1 = K1 * y           Y_2 = K1 * z                          Y_3 = K1 * x
 *     Y_4 = (K2 * x) * y                       Y_5 = (K2 * y) * z
 *     Y_6 = K3 * (((3.0 * z) * z) - 1.0)       Y_7 = (K2 * x) * z                    Y_8 = K4 * ((x * x) - (y * y))
 *     K0 = 0.28209479177387814  K1 = 0.4886025119029199  K2 = 1.0925484305920792  K3 = 0.31539156525252005  K4 = 0.5462742152960396
 *
 * (the f64 nearest to sqrt(1/4pi), sqrt(3/4pi), sqrt(15/4pi), sqrt(5/16pi), sqrt(15/16pi)).
 *
 * The sums.  The samples are cut into chunks by sample_chunk's rule (RADIANCE QUERY's).  Per chunk j, C_j[k][ch] starts at +0
 * and, for each sample of the chunk in sample order, C_j[k][ch] = C_j[k][ch] + (Y_k * L_s[ch]): one multiplication, then one
 * addition.  The probe's sum is C_0 assigned, then += C_j in chunk order, and
 *
 *     coeffs[i][k][ch] = sum[k][ch] * (FOUR_PI * (1.0 / (double)S)),   FOUR_PI = 4.0 * RR_PI
 *
 * -- the Monte-Carlo estimate of the integral of L * Y_k over the sphere with the uniform density 1 / 4pi.  queries[i] is the
 * sum of the probe's paths' Bvh::intersect calls, shadow rays included.  NaN and infinite L_s are not laundered: they enter the
 * sums as they are, and a point with a NaN component gives NaN where its paths do.  max_bounces == 0 gives +0 and no query.
 *
 * The bits are these under any schedule: on the device a sample is one item of the lighting's wave (radiance_probe.hip starts
 * the direct, sky, mesh and tree wave with a start of its own), its L_s and count land in the scene's radiance scratch, and a
 * projection behind the wave -- a thread per (probe, chunk) that makes w again from the key, then a thread per coefficient that
 * adds the chunks -- forms the sums in the order above, with no atomic on an f64 and no scratch memory.  A launch takes whole
 * probes, n_launch * S <= 2^20.  The projection's chunk sums live in a buffer of FIXED size (2^15 (probe, chunk) pairs, 7,208,960
 * bytes), allocated at the scene's first probe call; a launch with more pairs than that is projected in rounds, so after that
 * call the _launch form allocates and copies nothing (a group's and the sky's table are uploaded at THEIR first device call).
 *
 * rayrs_scene_probes and its _launch form: `lights`, `n_lights` are DIRECT LIGHTING's list (at most RAYRS_MAX_LIGHTS objects,
 * n_lights == 0 is legal), `sky` is 0 or 1 as MESH LIGHTS' entry points take it, `mesh` is NULL, an area group or a tree group.
 * No group and no sky: DIRECT LIGHTING's wave (with an empty list: the unlit bits); sky: SKY SAMPLING's; a group of N >= 1: MESH
 * LIGHTS' or LIGHT TREE's by the handle's kind (an empty group is no group).  coeffs is n * 9 * 3 f64; queries (n u32) may be
 * NULL.  The _launch form takes device pointers and a stream under RADIANCE QUERY's ordering rule.  Refusals, all decided
 * before the device is touched, in this order: RAYRS_INVALID_ARG for a NULL scene, position or coeffs; for samples == 0, a
 * fast_traversal above 1 or a sky above 1; for what DIRECT LIGHTING calls invalid in a list (a NULL list with n_lights > 0, an
 * index that is no object); for a group of another scene.  Then RAYRS_UNSUPPORTED for samples > 2^20 or max_bounces > 8000; for
 * samples * (2 * max_bounces + 1) >= 2^32; for what DIRECT LIGHTING calls unsupported in a list (more than RAYRS_MAX_LIGHTS, a
 * triangle, its material rule) and, with sky = 1, SKY SAMPLING's empty table.  RAYRS_NO_DEVICE comes last; n == 0 is RAYRS_OK.
 *
 * Two calls on the host, which need no device: rayrs_probe_directions writes the w of every (i, s), i < n, s < samples, as
 * n * samples * 3 f64 (RAYRS_INVALID_ARG for a NULL out); rayrs_sh_basis the nine Y_k of m directions, m * 9 f64, NaN and
 * infinite components going through the formulas as they are.
 *
 * Out of scope: orders above 2; a bake or a film of probes; the command line; visibility or depth moments; rayrs_render_multi. */
int rayrs_scene_probes(rayrs_scene* scene, const double* position /* n*3 */, uint64_t n, uint32_t samples, uint32_t max_bounces,
                       uint32_t sample_chunk, uint64_t seed, uint64_t index_base, uint32_t fast_traversal, const uint32_t* lights,
                       uint32_t n_lights, const rayrs_mesh_lights* mesh /* may be NULL: no group */, uint32_t sky,
                       double* coeffs /* n*9*3 */, uint32_t* queries /* n, may be NULL */);
int rayrs_scene_probes_launch(rayrs_scene* scene, const double* position, uint64_t n, uint32_t samples, uint32_t max_bounces,
                              uint32_t sample_chunk, uint64_t seed, uint64_t index_base, uint32_t fast_traversal, const uint32_t* lights,
                              uint32_t n_lights, const rayrs_mesh_lights* mesh /* may be NULL: no group */, uint32_t sky,
                              double* coeffs /* n*9*3 */, uint32_t* queries /* n, may be NULL */, void* hip_stream);
int rayrs_probe_directions(uint64_t seed, uint64_t index_base, uint64_t n, uint32_t samples, double* out /* n*samples*3 */);
int rayrs_sh_basis(const double* direction /* m*3 */, uint64_t m, double* out /* m*9 */);

/* LIGHTMAP ATLAS.  The step before a BAKE of lightmap texels: a mesh's triangles, rasterised in the UV space of a W x H atlas into
 * the list of covered texels with their world positions and normals -- the points and normals rayrs_bake_create wants -- and the
 * way back, per-texel values assembled into an (H, W, C) image whose chart borders are dilated.  An atlas is bound to a mesh, a
 * UV layout, a size and a device, and to no scene (rayrs_history is the precedent); it outlives every scene.
 *
 * LIGHTMAP ATLAS, specified to the operation.  Everything is f64 `+ - * /` and comparisons, unfused, in the order written; every
 * condition is written in its positive form, so that a NaN takes the "no" side.  Inputs: verts, nv * 3 f32 (vert_is_f32 = 1,
 * each widened exactly, as rayrs_object_from_triangles_f32 widens) or f64; idx, m * 3 u32; uvs, PER CORNER, m * 3 * 2 f64
 * (u, v of corner c of triangle k at uvs[(k*3 + c)*2 ..]); W = width, H = height; flip.  Texel (x, y), 0 <= x < W, 0 <= y < H,
 * has the index y*W + x and its centre at px = (double)x + 0.5, py = (double)y + 0.5.
 *
 * COVERAGE.  For triangle k with corners (u_c, v_c), c = 0, 1, 2:
 *     U_c = u_c * (double)W,   V_c = v_c * (double)H
 *     w0(px, py) = (U2 - U1) * (py - V1) - (V2 - V1) * (px - U1)        the edge function opposite corner 0
 *     w1(px, py) = (U0 - U2) * (py - V2) - (V0 - V2) * (px - U2)        ... corner 1
 *     w2(px, py) = (U1 - U0) * (py - V0) - (V1 - V0) * (px - U0)        ... corner 2
 *     area2 = w2(U2, V2) = (U1 - U0) * (V2 - V0) - (V1 - V0) * (U2 - U0)
 * -- four differences, two products, one subtraction each.  If area2 < 0 the triangle is wound the other way: w0, w1, w2 and
 * area2 are negated (exactly).  A triangle of which some U_c or V_c is not finite, or whose area2 is not finite or == 0, covers
 * nothing.  Texel (x, y) is a CANDIDATE of k iff
 *     (double)(x + 1) >= Umin  &&  (double)x <= Umax  &&  (double)(y + 1) >= Vmin  &&  (double)y <= Vmax,
 * Umin, Umax, Vmin, Vmax the smallest and largest of the U_c and of the V_c (every texel whose centre lies in the triangle's
 * bounding box is one, and the rule is part of the operation so that no rounding of an edge function can reach outside it); k
 * COVERS a candidate iff w0 >= 0 && w1 >= 0 && w2 >= 0 at its centre.  UVs outside [0, 1] are legal: what lies outside the
 * atlas has no texel, nothing wraps.  The OWNER of a texel is the LOWEST k that covers it, RAYRS_LIGHTMAP_NO_OWNER (0xFFFFFFFF)
 * if none does: a centre on which the edge functions of two triangles that share the edge are both exactly 0 belongs to the
 * lower index and is lost by neither; of two triangles laid over each other the lower index wins.
 *
 * TEXEL RECORD of an owned texel, k its owner, P_c = verts[idx[k*3 + c]]:
 *     b1 = w1 / area2,   b2 = w2 / area2,   b0 = (1.0 - b1) - b2                     (after the negation, if any)
 *     position = (b0 * P0 + b1 * P1) + b2 * P2                                       per component
 *     normal   = Triangle::new's unit normal of (P0, P1, P2), geometry.rs:341-353, from the routine MESH LIGHTS' table uses on
 *                the host (radiance_mesh_table.h mesh_tri_finish): e1 = P1 - P0, e2 = P2 - P0, nrm = e1 x e2,
 *                n = nrm * (1.0 / rr_sqrt((nrm.x*nrm.x + nrm.y*nrm.y) + nrm.z*nrm.z)) -- the bits rayrs_scene_intersect reports
 *                for a hit on a triangle of these vertices, not flipped towards anything; each component negated if flip.
 * A triangle whose normal is not finite (no area in space) keeps its texels, with that normal: BAKE has its rules for a NaN
 * normal (which NaN it is, sign and payload, is not specified).  The TEXEL LIST is the owned texels in ascending texel index; n
 * is their number.
 *
 * ASSEMBLY of values (n rows of C channels, 1 <= C <= 4, row i belonging to list entry i) with dilate = d >= 0.  The image is
 * H * W * C f64, the validity plane H * W bytes.  Row i goes to texel index[i], which becomes valid (1); every other texel is
 * +0 and invalid (0).  Then d rounds of dilation.  In a round every invalid texel (x, y) with at least one valid texel --
 * valid BEFORE the round -- among its eight neighbours inside the atlas becomes valid, with, per channel,
 *     s = +0;  for dy = -1, 0, 1 (outer), dx = -1, 0, 1 (inner), the valid neighbours (x + dx, y + dy) in that order: s = s + value;
 *     value = s / (double)count
 * -- count the number of those neighbours.  Every other texel keeps its value and its validity.  NaN and infinite values
 * travel as values.  (A round that makes no texel valid ends the rounds: every later one would change nothing.)
 *
 * The bits are these under any schedule.  lightmap.hip's owner pass gives each lane of a wave one triangle: a lane walks the
 * candidates of a triangle with at most 64 of them itself; the wave's 64 lanes stride the candidates of each triangle of the
 * wave's with up to 65536; a triangle with more goes to a list that a second launch strides with the whole grid.  The only
 * write to the owner plane is an integer atomicMin of k; there is no atomic on an f64.  Then a stream compaction in texel order
 * (flag and count, a scan of the workgroups' counts), and the record pass, a thread per texel, forms w1, w2 and area2 again for
 * the owner and writes the record at the texel's place in the list.  Assembly is a scatter kernel and one dilation kernel over
 * two planes, run once per round.
 *
 * Refusals, in this order: RAYRS_INVALID_ARG for a NULL out or handle; for NULL verts, idx or uvs with m > 0; for vert_is_f32
 * or flip above 1; for a width or a height of 0 or above RAYRS_LIGHTMAP_MAX_SIDE (16384); for an idx entry >= nv; in
 * rayrs_lightmap_assemble for NULL values with n > 0 or a NULL image, channels outside 1..4, a negative dilate.  Then
 * RAYRS_NO_DEVICE where `device` is no HIP device of this machine (device = -1 among them).  m = 0 is legal and gives an empty
 * atlas (n = 0).  The calls on one atlas come from one thread at a time; two atlases share nothing.
 *
 * Out of scope: chart-preserving or angle-based unwrapping (rayrs_amd.unwrap_triangles lays triangles out one by one);
 * conservative (overlap) coverage and clamped barycentrics for border texels; supersampled texels and per-texel jitter;
 * interpolated vertex normals; a device-resident hand-over of the texel list to a bake; the command line; bilinear sampling of
 * the result; seam stitching across charts. */
typedef struct rayrs_lightmap rayrs_lightmap;
#define RAYRS_LIGHTMAP_NO_OWNER 0xFFFFFFFFu
#define RAYRS_LIGHTMAP_MAX_SIDE 16384u

int rayrs_lightmap_create(int device, const void* verts /* nv*3 */, uint32_t vert_is_f32, uint32_t nv, const uint32_t* idx /* m*3 */,
                          uint32_t m, const double* uvs /* m*3*2 */, uint32_t width, uint32_t height, uint32_t flip,
                          rayrs_lightmap** out);
void rayrs_lightmap_destroy(rayrs_lightmap* lightmap);
/* n, the length of the texel list. */
int rayrs_lightmap_count(const rayrs_lightmap* lightmap, uint64_t* n);
/* The texel list into host buffers, each of which may be NULL: the texel indices (n u32, ascending), the positions, the normals
 * and the barycentrics (b0, b1, b2) (n * 3 f64 each). */
int rayrs_lightmap_texels(rayrs_lightmap* lightmap, uint32_t* index, double* points, double* normals, double* bary);
/* The owner plane, H * W u32. */
int rayrs_lightmap_owner(rayrs_lightmap* lightmap, uint32_t* owner);
/* ASSEMBLY above: values n * channels f64 (host); image H * W * channels f64; valid H * W bytes, may be NULL. */
int rayrs_lightmap_assemble(rayrs_lightmap* lightmap, const double* values, uint32_t channels, int32_t dilate, double* image,
                            uint8_t* valid);

/* The boundary's version: bumped whenever a struct of this header changes the meaning of a field or an entry point
 * its behaviour.  5 = round 5: rayrs_render_params.exact_traversal became fast_traversal (opposite sense: zero is now
 * the reference's visit set), the device self-test hooks left this header.  6 = round 6: rayrs_scene_info_t.hot_*,
 * rayrs_render_stats.hot_*, rayrs_scene_export_hot_tree, rayrs_obj_load_spheres.  7: the progressive film (rayrs_film_*, rayrs_film_params,
 * rayrs_film_status; no existing struct changed); still 7 with rayrs_film_render_adaptive and rayrs_film_tile_samples: entry points
 * were added, no struct or existing call changed; and with rayrs_render_features, rayrs_film_features, rayrs_film_denoise and
 * rayrs_image_denoise, for the same reason, and with rayrs_film_noise, rayrs_film_denoise_guided and
 * rayrs_image_denoise_guided, and with rayrs_history_* and rayrs_camera_orbit (TEMPORAL ACCUMULATION), and with
 * rayrs_scene_intersect, rayrs_scene_occluded and their _launch forms (RAY QUERIES), and with
 * rayrs_scene_ambient_occlusion, its _launch form and rayrs_render_ao (AMBIENT OCCLUSION), and with rayrs_scene_radiance,
 * rayrs_scene_irradiance and their _launch forms (RADIANCE QUERY, IRRADIANCE), and with rayrs_scene_radiance_lit,
 * rayrs_scene_irradiance_lit, their _launch forms and rayrs_render_lit (LIGHT SAMPLING), and with rayrs_scene_radiance_direct,
 * rayrs_scene_irradiance_direct, their _launch forms and rayrs_render_direct (DIRECT LIGHTING), and with rayrs_scene_radiance_sky,
 * rayrs_scene_irradiance_sky, their _launch forms, rayrs_render_sky, rayrs_scene_sky_table, rayrs_scene_sky_sample and
 * rayrs_scene_sky_density (SKY SAMPLING), and with rayrs_film_create_direct and rayrs_film_create_sky (DIRECT-LIT FILMS), and with
 * rayrs_bake_* and its three structs (BAKE; they are not in the layout table below: all their fields are 4 or 8 bytes wide and
 * naturally aligned), and with rayrs_mesh_lights_*, rayrs_scene_radiance_mesh, rayrs_scene_irradiance_mesh, their _launch forms
 * and rayrs_render_mesh (MESH LIGHTS), and with rayrs_film_create_mesh and rayrs_bake_create_mesh (MESH-LIT FILMS AND BAKES), and with
 * rayrs_mesh_lights_create_tree and rayrs_mesh_lights_tree_* (LIGHT TREE), and with rayrs_scene_probes, its _launch form,
 * rayrs_probe_directions and rayrs_sh_basis (SH PROBES), and with rayrs_lightmap_* (LIGHTMAP ATLAS).  The layout table below begins with this
 * number, so a binding that checks itself against the table fails on a version change as well.  A binding MUST compare
 * rayrs_abi_version() with the RAYRS_ABI_VERSION it was written against when it loads the library.  Every struct a caller fills must be zero-initialised
 * first: fields are added where padding used to be, and values out of a field's range are refused. */
#define RAYRS_ABI_VERSION 7
uint32_t rayrs_abi_version(void);

/* ---- layout of the structs above as THIS library was compiled, for bindings in other languages
 * to check theirs against (tests/test_abi.py does it for rayrs_amd/_ffi.py, and INTEGRATION.md's
 * #[repr(C)] structs carry the same numbers).  Writes up to `cap` words to `out` and returns the
 * number of words the full table has: first RAYRS_ABI_VERSION, then for each struct, in the order rayrs_material,
 * rayrs_emission, rayrs_camera, rayrs_scene_info_t, rayrs_render_params, rayrs_render_stats,
 * rayrs_tuning, rayrs_film_params, rayrs_film_status: sizeof, number of fields, then offsetof of every field in declaration order. */
uint32_t rayrs_abi_layout(uint32_t* out, uint32_t cap);

/* ---- file formats either side of the path (host only) ---- */

const char* rayrs_io_last_error(void);
/* frees a buffer returned by one of the loaders below */
void rayrs_buffer_free(void* p);

/* PLY 1.0, ascii or binary_little_endian: element vertex {x,y,z (+ ignored properties)},
 * element face {list vertex_indices}; polygons are fan-triangulated, winding kept.
 * (The reference's `ply` crate is entirely commented out, ply/src/lib.rs:1-350, so this
 * follows the public format.)  verts: nverts*3 f32, idx: ntris*3 -- feed them to
 * rayrs_object_from_triangles_f32. */
int rayrs_ply_load(const char* path, float** verts, uint32_t* nverts, uint32_t** idx, uint32_t* ntris);
int rayrs_ply_save(const char* path, const float* verts, uint32_t nverts, const uint32_t* idx, uint32_t ntris,
                   int binary);
/* wavefront_obj::load_obj_file, wavefront_obj.rs:15-45: `v x y z` / `f i j k` lines only. */
int rayrs_obj_load(const char* path, double** verts, uint32_t* nverts, uint32_t** idx, uint32_t* ntris);
/* wavefront_obj::load_obj_file_spheres, wavefront_obj.rs:46-64: one sphere centre per `v x y z` line, every other line
 * skipped; centers: n*3 f64 -- with the radius, feed them to rayrs_object_from_spheres (Object::from_spheres, lib.rs:422). */
int rayrs_obj_load_spheres(const char* path, double** centers, uint32_t* n);
/* Radiance .hdr: what HdrDecoder / HDREncoder do at rayrs/src/main.rs:36-41 and :113-121.
 * rgb: w*h*3 f32, top row first. */
int rayrs_hdr_load(const char* path, float** rgb, uint32_t* w, uint32_t* h);
int rayrs_hdr_save(const char* path, const float* rgb, uint32_t w, uint32_t h);
/* Image::to_raw_bytes(gamma), image.rs:193-222: clip(0,1).powf(gamma), (255.99*x) as u8.
 * out: w*h*3 bytes; counts = {clamped, NaN, negative} pixels (image.rs:218-220). */
int rayrs_image_to_bytes(const float* rgb, uint32_t w, uint32_t h, double gamma, uint8_t* out, uint64_t counts[3]);
int rayrs_ppm_save(const char* path, const uint8_t* bytes, uint32_t w, uint32_t h); /* image.rs:248-251 */
int rayrs_png_save(const char* path, const uint8_t* bytes, uint32_t w, uint32_t h); /* main.rs:104-110 */

#ifdef __cplusplus
}
#endif
#endif
