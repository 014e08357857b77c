// rayrs_cli.cpp -- the reference's command line (rayrs/src/main.rs) on top of the C ABI:
//
//     rayrs hdri_path [spp] [--scene NAME] [--seed N] [--device N] [--max-bounces N] [--fast-traversal 0|1]
//                           [--gpus N | --devices a,b,...] [--sample-chunk C] [--pass N] [--until-noise TAU]
//                           [--denoise [LEVELS]] [--features] [--denoise-guided [LEVELS]] [--noise]
//                           [--ao [S]] [--ao-radius R] [--direct] [--sky]
//
// --direct and --sky make the film direct-lit (include/rayrs_hip.h DIRECT-LIT FILMS): --direct lists the scene's emissive spheres
// and rectangles that DIRECT LIGHTING's material rule admits, in object order, --sky adds the sky.  Both need a film (--pass or
// --until-noise); without one, with --direct on a scene that has no admissible lamp and no --sky, or with more than 8 lamps, the
// program prints a usage error naming the option, exits with status 2 and writes nothing.  Every other option works on such a film
// unchanged, and with neither option every file is the same bytes as without this paragraph.
//
// --ao additionally writes <scene>_ao.png (no gamma) and <scene>_ao.hdr: the ambient-occlusion plane of include/rayrs_hip.h
// (AMBIENT OCCLUSION PLANE) on three channels, S samples a pixel (default 16), ao_seed 0xA0, rays leaving the surface by a bias
// of 1e-6 of the root box's diagonal and reaching --ao-radius R (default: anywhere).  <scene>.png and <scene>.hdr are the same
// bytes with and without it.
//
// --denoise additionally writes <scene>_denoised.png and .hdr: the final frame (as f64) through the feature-guided a-trous
// filter of include/rayrs_hip.h (DENOISER), LEVELS levels (default 5), with the normal, albedo and depth of 16 samples and
// the starting-point sigmas of rayrs_amd/api.py (SIGMA_*).  --features additionally writes <scene>_normal.png
// (0.5 n + 0.5, no gamma), <scene>_albedo.png and <scene>_depth.hdr.  <scene>.png and <scene>.hdr are the same bytes
// with and without either.
//
// --denoise-guided additionally writes <scene>_guided.png and .hdr: the film's frame through the variance-guided filter of
// include/rayrs_hip.h (GUIDED FILTER), LEVELS levels (default 5), with the film's own noise plane, the same features and
// sigmas and a luminance sigma of 4 standard deviations.  --noise additionally writes <scene>_noise.hdr: the noise plane
// (NOISE PLANE) on three channels, converted to f32 (+infinity stays +infinity).  Both read a film's statistics, so they
// need --pass or --until-noise: without one the program prints a usage error, exits with status 2 and writes nothing.
//
// --sample-chunk C sums a pixel's samples in chunks of C (rayrs_render_params.sample_chunk; default 0: the reference's one
// sequential sum).  --pass N renders through a progressive film (rayrs_film_*) in passes of N samples, rounded up to a
// multiple of C, and rewrites the PNG and the HDR after each pass; --until-noise TAU stops once every finite pixel is
// converged at TAU (include/rayrs_hip.h NOISE), with spp as the upper limit, in passes of 16 unless --pass says otherwise.
// A film sums in chunks (C defaults to 4 with either option) and writes the files a plain render with the same
// --sample-chunk writes; with none of the three options the program does exactly what it did without them.
//
// --gpus N renders on HIP devices 0..N-1 at once (--devices names them; a device may be named more than
// once to rehearse on fewer GPUs): image tiles interleaved over the devices, one RCCL reduce of the
// framebuffer (rayrs_render_multi) -- the counterpart of the reference's rayon block loop, which also
// lives inside the binary.
//
// Same positional arguments and defaults as main.rs:125-138 (spp defaults to 2000 and a spp
// that does not parse silently becomes 2000), same default scene (material_test, main.rs:201),
// same outputs: <scene>.png (gamma 1/2.2) and <scene>.hdr, "Time taken" and the
// clamped/NaN/negative pixel counts.  The reference picks the scene by editing main();
// --scene selects among the same functions of test_scenes.rs.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rayrs_hip.h"
#include "layout.h"

namespace {

rayrs_material cook_torrance_metal(double r, double g, double b, double alpha, double r0r, double r0g, double r0b) {
    rayrs_material m;
    std::memset(&m, 0, sizeof m);
    m.kind = RAYRS_MAT_COOK_TORRANCE;
    m.metallic = 1;
    m.color[0] = r, m.color[1] = g, m.color[2] = b;
    m.alpha = alpha;
    m.r0[0] = r0r, m.r0[1] = r0g, m.r0[2] = r0b;
    return m;
}

rayrs_material simple(int kind, double c, double alpha = 0., double ior = 0.) {
    rayrs_material m;
    std::memset(&m, 0, sizeof m);
    m.kind = kind;
    m.color[0] = m.color[1] = m.color[2] = c;
    m.spec_color[0] = m.spec_color[1] = m.spec_color[2] = 1.0;
    m.alpha = alpha;
    m.ior = ior;
    return m;
}

struct SceneDef {
    std::vector<rayrs_material> spheres;  // one unit sphere per material
    double cam_origin[3], cam_lookat[3], fov, width, height;
    uint32_t ppi;
    bool row;  // multiple_spheres layout (test_scenes.rs:169-211) or single sphere (:14-44)
};

bool make_scene(const std::string& name, SceneDef& s) {
    s.spheres.clear();
    auto row_cam = [&](double oy, double fov, double h) {
        s.cam_origin[0] = 0, s.cam_origin[1] = oy, s.cam_origin[2] = 20;
        s.cam_lookat[0] = 0, s.cam_lookat[1] = 1, s.cam_lookat[2] = 0;
        s.fov = fov, s.width = 1920. / 500., s.height = h, s.ppi = 125, s.row = true;
    };
    auto single_cam = [&]() {
        s.cam_origin[0] = 0, s.cam_origin[1] = 5, s.cam_origin[2] = 10;
        s.cam_lookat[0] = 0, s.cam_lookat[1] = 1, s.cam_lookat[2] = 0;
        s.fov = 50., s.width = 1920. / 500., s.height = 1080. / 500., s.ppi = 100, s.row = false;
    };
    if (name == "material_test") {  // test_scenes.rs:276-331
        s.spheres = {simple(RAYRS_MAT_LAMBERTIAN, 0.8), simple(RAYRS_MAT_PLASTIC, 0.8, 0.05, 1.45),
                     simple(RAYRS_MAT_REFLECT, 0.8), cook_torrance_metal(1, 1, 1, 0.05, 0.8, 0.8, 0.8),
                     simple(RAYRS_MAT_GLASS, 1.0, 0., 1.45), simple(RAYRS_MAT_COOK_TORRANCE_GLASS, 1.0, 0.05, 1.45),
                     simple(RAYRS_MAT_NO_REFLECT, 0.)};
        row_cam(3., 90., 250. / 500.);
    } else if (name == "spheres_metallic") {  // :213-224
        for (int i = 0; i < 7; i++) s.spheres.push_back(cook_torrance_metal(1, 1, 1, 0.01 * (double)(4 * i + 1), 0.8, 0.8, 0.8));
        row_cam(10., 72., 400. / 500.);
    } else if (name == "spheres_plastic") {  // :226-239
        for (int i = 0; i < 7; i++) s.spheres.push_back(simple(RAYRS_MAT_PLASTIC, 0.8, 0.01 * (double)(4 * i + 1), 1.45));
        row_cam(10., 72., 400. / 500.);
    } else if (name == "cook_torrance_spheres_frosted_glass") {  // :241-256
        for (int i = 0; i < 7; i++)
            s.spheres.push_back(simple(RAYRS_MAT_COOK_TORRANCE_GLASS, 1.0, 0.01 * (double)(4 * i + 1), 1.45));
        row_cam(10., 72., 400. / 500.);
    } else if (name == "diffuse_single_sphere") {  // :60-63
        s.spheres = {simple(RAYRS_MAT_LAMBERTIAN, 0.8)};
        single_cam();
    } else if (name == "copper_sphere") {  // :46-53
        s.spheres = {cook_torrance_metal(1, 1, 1, 0.05, 0.722, 0.451, 0.2)};
        single_cam();
    } else if (name == "glass_sphere") {  // :55-58
        s.spheres = {simple(RAYRS_MAT_GLASS, 0.8, 0., 1.45)};
        single_cam();
    } else if (name == "cook_torrance_glass_sphere") {  // :65-68
        s.spheres = {simple(RAYRS_MAT_COOK_TORRANCE_GLASS, 0.8, 0.05, 1.45)};
        single_cam();
    } else {
        return false;
    }
    return true;
}

int fail(const char* what, int status) {
    std::fprintf(stderr, "%s: %s (%s %s)\n", what, rayrs_strerror(status), rayrs_last_error(), rayrs_io_last_error());
    return 1;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {  // main.rs:126-128
        std::fprintf(stderr, "Usage: rayrs hdri_path [spp]\n");
        return 1;
    }
    const char* hdri_path = argv[1];
    uint32_t spp = 2000;  // SPP, main.rs:20
    std::string scene_name = "material_test";
    uint64_t seed = 0x5EED;
    int device = 0;
    uint32_t max_bounces = 50;  // main.rs:77
    uint32_t fast_traversal = 0;  // rayrs_render_params.fast_traversal: 0 = the reference's visit set by construction
    uint32_t sample_chunk = 0, pass = 0;
    bool chunk_given = false, until_noise = false, adaptive = false;
    double tau = 0.0;
    bool want_denoise = false, want_features = false;
    uint32_t denoise_levels = 5;
    bool want_guided = false, want_noise = false;
    uint32_t guided_levels = 5;
    bool want_direct = false, want_sky = false;  // --direct, --sky: a direct-lit film
    bool want_ao = false;
    uint32_t ao_samples = 16;
    double ao_radius = INFINITY;
    constexpr uint64_t AO_SEED = 0xA0;  // rayrs_amd/api.py render_ao's default
    constexpr double AO_BIAS_FRACTION = 1e-6;
    uint32_t orbit_frames = 0;  // --orbit FRAMES DEGREES: frame i from the camera turned by i * DEGREES / FRAMES about its up through its lookat
    double orbit_degrees = 0.0;
    bool orbit_given = false, temporal = false;  // --temporal: every frame's film is pushed into one history
    // starting points, as rayrs_amd/api.py TEMPORAL_*: the history's weight cap in samples, relative depth and normal tolerance
    constexpr double TEMPORAL_MAX_SAMPLES = 256.0, TEMPORAL_DEPTH_TOL = 0.02, TEMPORAL_NORMAL_TOL = 0.25;
    constexpr double SIGMA_LUMINANCE = 4.0;  // rayrs_amd/api.py SIGMA_LUMINANCE: SVGF's, in standard deviations of the pixel
    constexpr uint32_t FEATURE_SAMPLES = 16;
    // starting points chosen by eye, as rayrs_amd/api.py SIGMA_*: normal, albedo, depth as a fraction of the root-box diagonal, colour
    constexpr double SIGMA_NORMAL = 0.25, SIGMA_ALBEDO = 0.1, SIGMA_DEPTH_FRACTION = 0.02, SIGMA_COLOR = 0.6;
    std::vector<int> devices;
    int i = 2;
    if (i < argc && argv[i][0] != '-') {
        char* end = nullptr;
        const unsigned long v = std::strtoul(argv[i], &end, 10);
        if (end != argv[i] && *end == '\0' && v > 0) spp = (uint32_t)v;  // unwrap_or_else(|_| SPP), main.rs:133
        i++;
    }
    for (; i < argc; i += 2) {
        const std::string opt = argv[i];
        if (opt == "--adaptive") {  // the one option without a value
            adaptive = true;
            i--;
            continue;
        }
        if (opt == "--features") {
            want_features = true;
            i--;
            continue;
        }
        if (opt == "--noise") {
            want_noise = true;
            i--;
            continue;
        }
        if (opt == "--temporal") {
            temporal = true;
            i--;
            continue;
        }
        if (opt == "--direct" || opt == "--sky") {
            (opt == "--direct" ? want_direct : want_sky) = true;
            i--;
            continue;
        }
        if (opt == "--orbit") {  // two values
            orbit_given = true;
            if (i + 2 < argc) {
                orbit_frames = (uint32_t)std::strtoul(argv[i + 1], nullptr, 10);
                orbit_degrees = std::strtod(argv[i + 2], nullptr);
            }
            i++;
            continue;
        }
        if (opt == "--denoise-guided") {  // the level count is optional
            want_guided = true;
            char* end = nullptr;
            const unsigned long v = i + 1 < argc ? std::strtoul(argv[i + 1], &end, 10) : 0ul;
            if (i + 1 < argc && end != argv[i + 1] && *end == '\0') guided_levels = (uint32_t)v;
            else i--;
            continue;
        }
        if (opt == "--ao") {  // the sample count is optional
            want_ao = true;
            char* end = nullptr;
            const unsigned long v = i + 1 < argc ? std::strtoul(argv[i + 1], &end, 10) : 0ul;
            if (i + 1 < argc && end != argv[i + 1] && *end == '\0') ao_samples = (uint32_t)v;
            else i--;
            continue;
        }
        if (opt == "--denoise") {  // the level count is optional
            want_denoise = true;
            char* end = nullptr;
            const unsigned long v = i + 1 < argc ? std::strtoul(argv[i + 1], &end, 10) : 0ul;
            if (i + 1 < argc && end != argv[i + 1] && *end == '\0') denoise_levels = (uint32_t)v;
            else i--;
            continue;
        }
        if (i + 1 >= argc) break;
        if (opt == "--scene") scene_name = argv[i + 1];
        else if (opt == "--seed") seed = std::strtoull(argv[i + 1], nullptr, 0);
        else if (opt == "--device") device = std::atoi(argv[i + 1]);
        else if (opt == "--max-bounces") max_bounces = (uint32_t)std::atoi(argv[i + 1]);
        else if (opt == "--fast-traversal") fast_traversal = std::atoi(argv[i + 1]) ? 1u : 0u;
        else if (opt == "--exact-traversal") fast_traversal = std::atoi(argv[i + 1]) ? 0u : 1u;  // (the pre-round-5 spelling)
        else if (opt == "--sample-chunk") sample_chunk = (uint32_t)std::strtoul(argv[i + 1], nullptr, 10), chunk_given = true;
        else if (opt == "--pass") pass = (uint32_t)std::strtoul(argv[i + 1], nullptr, 10);
        else if (opt == "--until-noise") tau = std::strtod(argv[i + 1], nullptr), until_noise = true;
        else if (opt == "--ao-radius") ao_radius = std::strtod(argv[i + 1], nullptr);
        else if (opt == "--gpus") {
            devices.clear();
            for (int d = 0; d < std::atoi(argv[i + 1]); d++) devices.push_back(d);
        } else if (opt == "--devices") {
            devices.clear();
            for (const char* p = argv[i + 1]; *p;) {
                char* end = nullptr;
                devices.push_back((int)std::strtol(p, &end, 10));
                if (end == p) {
                    std::fprintf(stderr, "bad device list %s\n", argv[i + 1]);
                    return 1;
                }
                p = *end == ',' ? end + 1 : end;
            }
        }
        else {
            std::fprintf(stderr, "unknown option %s\n", opt.c_str());
            return 1;
        }
    }
    const bool use_film = pass != 0 || until_noise;
    if (use_film && !devices.empty()) {
        std::fprintf(stderr, "--pass / --until-noise render through a film, which is single-device: use --device, not --gpus / --devices\n");
        return 1;
    }
    if (adaptive && !until_noise) {
        std::fprintf(stderr, "--adaptive samples the tiles that are still noisy at a tau: give --until-noise TAU\n");
        return 1;
    }
    if ((want_guided || want_noise) && !use_film) {
        std::fprintf(stderr, "Usage: --denoise-guided and --noise read a film's noise estimate: give --pass N (or --until-noise TAU)\n");
        return 2;
    }
    if ((want_direct || want_sky) && !use_film) {
        std::fprintf(stderr, "Usage: %s makes the film direct-lit: give --pass N (or --until-noise TAU)\n", want_direct ? "--direct" : "--sky");
        return 2;
    }
    if ((orbit_given || temporal) && (!use_film || pass == 0)) {
        std::fprintf(stderr, "Usage: --orbit FRAMES DEGREES and --temporal render every frame through a film: give --pass N\n");
        return 2;
    }
    if (temporal && !orbit_given) {
        std::fprintf(stderr, "Usage: --temporal accumulates the frames of an orbit: give --orbit FRAMES DEGREES\n");
        return 2;
    }
    if (orbit_given && (orbit_frames == 0 || !std::isfinite(orbit_degrees))) {
        std::fprintf(stderr, "Usage: --orbit FRAMES DEGREES, FRAMES >= 1\n");
        return 2;
    }
    if (want_ao && ao_samples == 0) {
        std::fprintf(stderr, "Usage: --ao [S], S >= 1\n");
        return 2;
    }
    if (orbit_given && (adaptive || until_noise || want_features || want_noise || want_denoise || want_ao)) {
        std::fprintf(stderr, "Usage: --orbit writes each frame, with --temporal the history and with --denoise-guided the filtered one; it takes no other extra\n");
        return 2;
    }
    if (use_film && (!chunk_given || sample_chunk == 0)) sample_chunk = 4;
    if (use_film) {
        if (pass == 0) pass = 16;
        pass = (uint32_t)(((uint64_t)pass + sample_chunk - 1) / sample_chunk * sample_chunk);  // an open film takes whole chunks
    }
    SceneDef def;
    if (!make_scene(scene_name, def)) {
        std::fprintf(stderr, "unknown scene %s\n", scene_name.c_str());
        return 1;
    }

    float* hdri = nullptr;
    uint32_t hw = 0, hh = 0;
    int st = rayrs_hdr_load(hdri_path, &hdri, &hw, &hh);  // main.rs:36-41; the clip(0,3) of :43 happens in rayrs_scene_new
    if (st != RAYRS_OK) return fail("hdri", st);

    // --direct's list: the emissive spheres and rectangles, in object order, whose material always scatters (DIRECT LIGHTING's rule)
    std::vector<uint32_t> lamps;
    uint32_t n_objects = 0;
    auto note_object = [&](const rayrs_material& m, const rayrs_emission& e) {
        const bool emits = e.emissive != 0 && (e.strength * e.color[0] != 0.0 || e.strength * e.color[1] != 0.0 || e.strength * e.color[2] != 0.0);
        const bool always_scatters = m.kind == RAYRS_MAT_LAMBERTIAN || m.kind == RAYRS_MAT_REFLECT || m.kind == RAYRS_MAT_GLASS;
        if (emits && always_scatters) lamps.push_back(n_objects);
        n_objects++;
    };
    if (want_direct || want_sky) {  // (before anything is made: a usage error leaves nothing behind)
        rayrs_emission none;
        std::memset(&none, 0, sizeof none);
        note_object(cook_torrance_metal(1, 1, 1, 0.5, 0.8, 0.8, 0.8), none);
        for (const rayrs_material& m : def.spheres) note_object(m, none);
        if (!want_direct) lamps.clear();
        if (want_direct && lamps.empty() && !want_sky) {
            std::fprintf(stderr, "Usage: --direct needs a lamp, and scene %s has no emissive sphere or rectangle it can list: give --sky\n", scene_name.c_str());
            return 2;
        }
        if (lamps.size() > RAYRS_MAX_LIGHTS) {
            std::fprintf(stderr, "Usage: --direct lists at most %d lamps, scene %s has %zu\n", RAYRS_MAX_LIGHTS, scene_name.c_str(), lamps.size());
            return 2;
        }
    }

    rayrs_objects* objs = nullptr;
    if ((st = rayrs_objects_create(&objs)) != RAYRS_OK) return fail("objects", st);
    rayrs_emission dark;
    std::memset(&dark, 0, sizeof dark);
    const rayrs_material floor = cook_torrance_metal(1, 1, 1, 0.5, 0.8, 0.8, 0.8);  // test_scenes.rs:15-19
    if ((st = rayrs_object_plane(objs, RAYRS_AXIS_Y, -25., 25., -25., 25., 0., &floor, &dark)) != RAYRS_OK)
        return fail("floor", st);
    const long n = (long)def.spheres.size();
    for (long k = 0; k < n; k++) {
        const double origin[3] = {def.row ? 2.2 * (double)(k - n / 2) : 0.0, 1.0, 0.0};  // test_scenes.rs:184
        if ((st = rayrs_object_sphere(objs, 1., origin, &def.spheres[(size_t)k], &dark)) != RAYRS_OK)
            return fail("sphere", st);
    }
    if (devices.empty()) devices.push_back(device);
    rayrs_scene* scene = nullptr;
    st = rayrs_scene_new(objs, 0.000001, 1000000., RAYRS_BVH_SAH, 1000, hw, hh, hdri, devices[0], &scene);  // main.rs:52
    rayrs_objects_destroy(objs);
    rayrs_buffer_free(hdri);
    if (st != RAYRS_OK) return fail("scene", st);
    std::vector<rayrs_scene*> scenes{scene};  // one handle per device; the BVH is built once
    for (size_t d = 1; d < devices.size(); d++) {
        rayrs_scene* clone = nullptr;
        if ((st = rayrs_scene_clone_to_device(scene, devices[d], &clone)) != RAYRS_OK) return fail("scene clone", st);
        scenes.push_back(clone);
    }

    rayrs_camera cam;
    const double up[3] = {0., 1., 0.};
    if ((st = rayrs_camera_new(def.cam_origin, up, def.cam_lookat, def.fov, def.width, def.height, def.ppi, &cam)) != RAYRS_OK)
        return fail("camera", st);

    rayrs_render_params params;
    std::memset(&params, 0, sizeof params);
    params.spp = spp;
    params.max_bounces = max_bounces;
    params.seed = seed;
    params.sample_chunk = sample_chunk;  // 0 (the default): the reference's single sequential sum per pixel
    params.tile_rank = 0;
    params.tile_ranks = 1;
    params.out_format = RAYRS_OUT_F32;
    params.fast_traversal = fast_traversal;
    const size_t npix = (size_t)cam.x_pixels * cam.y_pixels;
    std::vector<float> rgb(npix * 3, 0.f);
    std::vector<uint8_t> bytes(rgb.size());
    // --denoise filters the f64 frame: a plain render is then asked for f64 and converted here, which is the conversion
    // the f32 output format makes at its store -- the same <scene>.png and <scene>.hdr
    std::vector<double> rgb64(want_denoise && !use_film ? npix * 3 : 0);
    std::vector<float> extra(want_denoise || want_features || want_guided || want_noise || temporal || want_ao ? npix * 3 : 0);
    auto write_extra = [&](const char* suffix, double gamma, bool png) -> int {
        const std::string name = scene_name + suffix + (png ? ".png" : ".hdr");
        if (!png) return rayrs_hdr_save(name.c_str(), extra.data(), cam.x_pixels, cam.y_pixels);
        uint64_t counts[3];
        rayrs_image_to_bytes(extra.data(), cam.x_pixels, cam.y_pixels, gamma, bytes.data(), counts);
        return rayrs_png_save(name.c_str(), bytes.data(), cam.x_pixels, cam.y_pixels);
    };
    double kn = 1.0 / (SIGMA_NORMAL * SIGMA_NORMAL), ka = 1.0 / (SIGMA_ALBEDO * SIGMA_ALBEDO), kc = 1.0 / (SIGMA_COLOR * SIGMA_COLOR), kz = 0.0;
    double ao_bias = 0.0;
    {
        rayrs_scene_info_t info;
        if ((st = rayrs_scene_info(scene, &info)) != RAYRS_OK) return fail("scene info", st);
        const double* b = info.root_box;
        const double dx = b[1] - b[0], dy = b[3] - b[2], dz = b[5] - b[4];
        const double diag = std::sqrt(dx * dx + dy * dy + dz * dz);
        if (std::isfinite(diag) && diag > 0.0) {
            const double sigma = SIGMA_DEPTH_FRACTION * diag;
            kz = 1.0 / (sigma * sigma);
            ao_bias = AO_BIAS_FRACTION * diag;
        }
    }
    // the feature files, from the planes of FEATURE_SAMPLES samples
    auto write_features = [&](const std::vector<double>& normal, const std::vector<double>& albedo, const std::vector<double>& depth) -> int {
        int s;
        for (size_t k = 0; k < npix * 3; k++) extra[k] = (float)(0.5 * normal[k] + 0.5);
        if ((s = write_extra("_normal", 1.0, true)) != RAYRS_OK) return fail("normal png", s), s;
        for (size_t k = 0; k < npix * 3; k++) extra[k] = (float)albedo[k];
        if ((s = write_extra("_albedo", 1. / 2.2, true)) != RAYRS_OK) return fail("albedo png", s), s;
        for (size_t k = 0; k < npix; k++) extra[3 * k] = extra[3 * k + 1] = extra[3 * k + 2] = (float)depth[k];
        if ((s = write_extra("_depth", 1.0, false)) != RAYRS_OK) return fail("depth hdr", s), s;
        return RAYRS_OK;
    };
    auto write_denoised = [&]() -> int {  // extra holds the filtered frame as f32
        int s;
        if ((s = write_extra("_denoised", 1. / 2.2, true)) != RAYRS_OK) return fail("denoised png", s), s;
        if ((s = write_extra("_denoised", 1.0, false)) != RAYRS_OK) return fail("denoised hdr", s), s;
        return RAYRS_OK;
    };
    // <scene>.png (gamma 1/2.2) and <scene>.hdr from rgb; the counts of image.rs:218-220 once, for the final frame
    auto write_files = [&](bool final_frame) -> int {
        uint64_t counts[3];
        rayrs_image_to_bytes(rgb.data(), cam.x_pixels, cam.y_pixels, 1. / 2.2, bytes.data(), counts);  // main.rs:106
        if (final_frame)
            std::printf("Clamped pixels: %llu\nNaN pixels: %llu\nNegative pixels: %llu\n", (unsigned long long)counts[0],
                        (unsigned long long)counts[1], (unsigned long long)counts[2]);  // image.rs:218-220
        int s = rayrs_png_save((scene_name + ".png").c_str(), bytes.data(), cam.x_pixels, cam.y_pixels);
        if (s != RAYRS_OK) return fail("png", s), s;
        if ((s = rayrs_hdr_save((scene_name + ".hdr").c_str(), rgb.data(), cam.x_pixels, cam.y_pixels)) != RAYRS_OK) return fail("hdr", s), s;
        return RAYRS_OK;
    };
    // the film of the options: plain, or direct-lit with --direct's lamps and, with --sky, the sky
    auto make_film = [&](const rayrs_film_params* fprm, rayrs_film** film) -> int {
        const uint32_t* list = lamps.empty() ? nullptr : lamps.data();
        if (want_sky) return rayrs_film_create_sky(scene, &cam, fprm, list, (uint32_t)lamps.size(), film);
        if (want_direct) return rayrs_film_create_direct(scene, &cam, fprm, list, (uint32_t)lamps.size(), film);
        return rayrs_film_create(scene, &cam, fprm, film);
    };
    if (orbit_given) {
        // <scene>_%04d.png/.hdr per frame; --temporal: <scene>_%04d_temporal.*, the history after the frame's push;
        // --denoise-guided: <scene>_%04d_guided.*, the history (--temporal) or the frame's film through the guided filter
        const std::string base = scene_name;
        const rayrs_camera cam0 = cam;
        const double kv = 1.0 / (SIGMA_LUMINANCE * SIGMA_LUMINANCE);
        rayrs_history* history = nullptr;
        if (temporal && (st = rayrs_history_create(devices[0], &history)) != RAYRS_OK) return fail("history", st);
        for (uint32_t frame = 0; frame < orbit_frames; frame++) {
            char tag[16];
            std::snprintf(tag, sizeof tag, "_%04u", frame);
            scene_name = base + tag;
            double origin[3];
            if ((st = rayrs_camera_orbit(def.cam_origin, up, def.cam_lookat, ((double)frame * orbit_degrees) / (double)orbit_frames, origin)) != RAYRS_OK)
                return fail("orbit", st);
            if ((st = rayrs_camera_new(origin, up, def.cam_lookat, def.fov, def.width, def.height, def.ppi, &cam)) != RAYRS_OK)
                return fail("camera", st);
            if (cam.x_pixels != cam0.x_pixels || cam.y_pixels != cam0.y_pixels) return fail("camera", RAYRS_INVALID_ARG);
            rayrs_film_params fprm;
            std::memset(&fprm, 0, sizeof fprm);
            fprm.sample_chunk = sample_chunk, fprm.max_bounces = max_bounces, fprm.seed = seed, fprm.fast_traversal = fast_traversal;
            rayrs_film* film = nullptr;
            if ((st = make_film(&fprm, &film)) != RAYRS_OK) return fail("film", st);
            for (uint32_t done = 0; done < spp;) {
                const uint32_t n = spp - done < pass ? spp - done : pass;
                if ((st = rayrs_film_render(film, n, nullptr)) != RAYRS_OK) return fail("film pass", st);
                done += n;
            }
            if ((st = rayrs_film_read(film, RAYRS_OUT_F32, rgb.data())) != RAYRS_OK) return fail("film read", st);
            if (write_files(false) != RAYRS_OK) return 1;
            if (temporal) {
                if ((st = rayrs_history_push_film(history, film, FEATURE_SAMPLES, TEMPORAL_MAX_SAMPLES, TEMPORAL_DEPTH_TOL, TEMPORAL_NORMAL_TOL)) != RAYRS_OK)
                    return fail("history push", st);
                if ((st = rayrs_history_read(history, RAYRS_OUT_F32, extra.data(), nullptr, nullptr)) != RAYRS_OK) return fail("history read", st);
                if ((st = write_extra("_temporal", 1. / 2.2, true)) != RAYRS_OK) return fail("temporal png", st);
                if ((st = write_extra("_temporal", 1.0, false)) != RAYRS_OK) return fail("temporal hdr", st);
            }
            if (want_guided) {
                st = temporal ? rayrs_history_denoise_guided(history, guided_levels, kn, ka, kz, kv, RAYRS_OUT_F32, extra.data(), nullptr)
                              : rayrs_film_denoise_guided(film, FEATURE_SAMPLES, guided_levels, kn, ka, kz, kv, RAYRS_OUT_F32, extra.data(), nullptr);
                if (st != RAYRS_OK) return fail("denoise guided", st);
                if ((st = write_extra("_guided", 1. / 2.2, true)) != RAYRS_OK) return fail("guided png", st);
                if ((st = write_extra("_guided", 1.0, false)) != RAYRS_OK) return fail("guided hdr", st);
            }
            rayrs_film_destroy(film);
            std::printf("Frame %u of %u: %.6g degrees\n", frame + 1, orbit_frames, ((double)frame * orbit_degrees) / (double)orbit_frames);
        }
        rayrs_history_destroy(history);
        for (rayrs_scene* sc : scenes) rayrs_scene_destroy(sc);
        return 0;
    }
    rayrs_render_stats stats;
    std::memset(&stats, 0, sizeof stats);
    const auto t0 = std::chrono::steady_clock::now();
    if (use_film) {
        rayrs_film_params fprm;
        std::memset(&fprm, 0, sizeof fprm);
        fprm.sample_chunk = sample_chunk;
        fprm.max_bounces = max_bounces;
        fprm.seed = seed;
        fprm.fast_traversal = fast_traversal;
        rayrs_film* film = nullptr;
        if ((st = make_film(&fprm, &film)) != RAYRS_OK) return fail("film", st);
        rayrs_film_status fs;
        std::memset(&fs, 0, sizeof fs);
        uint32_t done = 0;
        // --adaptive: passes over the tiles that still hold an unconverged pixel, none beyond spp samples, until every
        // finite pixel is converged or no tile is left to take a pass (rayrs_amd.render_until(adaptive=True))
        while (adaptive) {
            if ((st = rayrs_film_status_get(film, tau, &fs)) != RAYRS_OK) return fail("film status", st);
            if (fs.samples > 0 && fs.unconverged == 0) break;
            uint64_t active = 0;
            rayrs_render_stats ps;
            if (spp < pass) break;
            if ((st = rayrs_film_render_adaptive(film, pass, tau, spp, &active, &ps)) != RAYRS_OK) return fail("film pass", st);
            if (active == 0) break;
            if ((st = rayrs_film_read(film, RAYRS_OUT_F32, rgb.data())) != RAYRS_OK) return fail("film read", st);
            if ((st = rayrs_film_status_get(film, tau, &fs)) != RAYRS_OK) return fail("film status", st);
            std::printf("Pass: %llu active tiles, at most %llu samples, %llu pixels unconverged, %llu not finite\n",
                        (unsigned long long)active, (unsigned long long)fs.samples, (unsigned long long)fs.unconverged,
                        (unsigned long long)fs.nonfinite);
            if (write_files(false) != RAYRS_OK) return 1;
        }
        if (adaptive) {
            std::vector<uint32_t> per_tile((size_t)rayrs_film_tile_samples(film, nullptr, 0));
            rayrs_film_tile_samples(film, per_tile.data(), per_tile.size());
            const uint32_t tiles_x = rayrs::tile_share(cam.x_pixels, cam.y_pixels, 0u, 1u).tiles_x;
            uint64_t lo = ~0ull, hi = 0, sum = 0;
            for (uint32_t r = 0; r < cam.y_pixels; r++)
                for (uint32_t c = 0; c < cam.x_pixels; c++) {
                    const uint64_t v = per_tile[(size_t)(r / 8u) * tiles_x + c / 8u];
                    lo = v < lo ? v : lo, hi = v > hi ? v : hi, sum += v;
                }
            std::printf("Samples per pixel: min %llu, mean %.3f, max %llu\n", (unsigned long long)lo,
                        (double)sum / ((double)cam.x_pixels * cam.y_pixels), (unsigned long long)hi);
            if (hi == 0) return fail("film pass", RAYRS_INVALID_ARG);  // (spp below one pass: nothing was rendered)
            done = spp;
        }
        while (done < spp) {
            const uint32_t n = spp - done < pass ? spp - done : pass;  // (a short last pass closes the film: it is the last)
            rayrs_render_stats ps;
            if ((st = rayrs_film_render(film, n, &ps)) != RAYRS_OK) return fail("film pass", st);
            done += n;
            if ((st = rayrs_film_read(film, RAYRS_OUT_F32, rgb.data())) != RAYRS_OK) return fail("film read", st);
            if ((st = rayrs_film_status_get(film, tau, &fs)) != RAYRS_OK) return fail("film status", st);
            std::printf("Pass: %u of %u samples, %llu pixels unconverged, %llu not finite\n", done, spp,
                        (unsigned long long)fs.unconverged, (unsigned long long)fs.nonfinite);
            if (done < spp && write_files(false) != RAYRS_OK) return 1;
            if (until_noise && fs.unconverged == 0) break;
        }
        if (!adaptive) std::printf("Samples per pixel: %u\n", done);
        stats.rays = fs.rays, stats.paths = fs.paths, stats.nan_pixels = fs.nan_pixels, stats.neg_pixels = fs.neg_pixels;
        if (want_features) {
            std::vector<double> normal(npix * 3), albedo(npix * 3), depth(npix);
            if ((st = rayrs_film_features(film, FEATURE_SAMPLES, normal.data(), albedo.data(), depth.data(), nullptr, nullptr)) != RAYRS_OK)
                return fail("film features", st);
            if (write_features(normal, albedo, depth) != RAYRS_OK) return 1;
        }
        if (want_denoise) {
            if ((st = rayrs_film_denoise(film, FEATURE_SAMPLES, denoise_levels, kn, ka, kz, kc, RAYRS_OUT_F32, extra.data())) != RAYRS_OK)
                return fail("film denoise", st);
            if (write_denoised() != RAYRS_OK) return 1;
        }
        if (want_guided) {
            const double kv = 1.0 / (SIGMA_LUMINANCE * SIGMA_LUMINANCE);
            if ((st = rayrs_film_denoise_guided(film, FEATURE_SAMPLES, guided_levels, kn, ka, kz, kv, RAYRS_OUT_F32, extra.data(), nullptr)) != RAYRS_OK)
                return fail("film denoise guided", st);
            int s;
            if ((s = write_extra("_guided", 1. / 2.2, true)) != RAYRS_OK) return fail("guided png", s);
            if ((s = write_extra("_guided", 1.0, false)) != RAYRS_OK) return fail("guided hdr", s);
        }
        if (want_noise) {
            std::vector<double> plane(npix);
            if ((st = rayrs_film_noise(film, plane.data())) != RAYRS_OK) return fail("film noise", st);
            for (size_t k = 0; k < npix; k++) extra[3 * k] = extra[3 * k + 1] = extra[3 * k + 2] = (float)plane[k];
            int s;
            if ((s = write_extra("_noise", 1.0, false)) != RAYRS_OK) return fail("noise hdr", s);
        }
        rayrs_film_destroy(film);
    } else {
        if (want_denoise) params.out_format = RAYRS_OUT_F64;
        void* frame = want_denoise ? (void*)rgb64.data() : (void*)rgb.data();
        if (scenes.size() == 1)
            st = rayrs_render(scene, &cam, &params, frame, &stats);
        else
            st = rayrs_render_multi(scenes.data(), (uint32_t)scenes.size(), &cam, &params, frame, &stats);
        if (want_denoise)
            for (size_t k = 0; k < npix * 3; k++) rgb[k] = (float)rgb64[k];  // image.rs:224-229
    }
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (st != RAYRS_OK) return fail("render", st);
    if (stats.nan_pixels) std::fprintf(stderr, "NaN pixel detected\n");       // main.rs:81-83
    if (stats.neg_pixels) std::fprintf(stderr, "Negative pixel detected\n");  // main.rs:85-87
    std::printf("Time taken %s: %.3f s\n", scene_name.c_str(), secs);         // main.rs:96-100
    std::printf("Rays: %llu (%.1f Mray/s)\n", (unsigned long long)stats.rays, (double)stats.rays / secs / 1e6);

    if (write_files(true) != RAYRS_OK) return 1;
    if (!use_film && (want_denoise || want_features)) {
        std::vector<double> normal(npix * 3), albedo(npix * 3), depth(npix);
        if ((st = rayrs_render_features(scene, &cam, FEATURE_SAMPLES, seed, 0, 1, fast_traversal, normal.data(), albedo.data(),
                                        depth.data(), nullptr, nullptr)) != RAYRS_OK)
            return fail("features", st);
        if (want_features && write_features(normal, albedo, depth) != RAYRS_OK) return 1;
        if (want_denoise) {
            std::vector<double> out64(npix * 3);
            if ((st = rayrs_image_denoise(devices[0], cam.x_pixels, cam.y_pixels, rgb64.data(), normal.data(), albedo.data(),
                                          depth.data(), denoise_levels, kn, ka, kz, kc, out64.data())) != RAYRS_OK)
                return fail("denoise", st);
            for (size_t k = 0; k < npix * 3; k++) extra[k] = (float)out64[k];
            if (write_denoised() != RAYRS_OK) return 1;
        }
    }
    if (want_ao) {
        std::vector<double> vis(npix);
        if ((st = rayrs_render_ao(scene, &cam, seed, AO_SEED, ao_samples, ao_radius, ao_bias, fast_traversal, nullptr, vis.data())) != RAYRS_OK)
            return fail("ao", st);
        for (size_t k = 0; k < npix; k++) extra[3 * k] = extra[3 * k + 1] = extra[3 * k + 2] = (float)vis[k];
        if ((st = write_extra("_ao", 1.0, true)) != RAYRS_OK) return fail("ao png", st);
        if ((st = write_extra("_ao", 1.0, false)) != RAYRS_OK) return fail("ao hdr", st);
    }
    for (rayrs_scene* sc : scenes) rayrs_scene_destroy(sc);
    return 0;
}
