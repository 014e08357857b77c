"""Scenes, HDRIs and the frame comparison of the non-finite tests (test_nonfinite_oracle.py on the CPU,
test_gpu_nonfinite.py on the GPU).

Every surface parameter here passes the reference's constructor asserts (and scene_host.cpp add_surface, which
copies them), yet drives the path into NaN, infinite, huge or f32-subnormal radiance: alpha whose square underflows
or overflows, emission strengths of inf, 1e308 and 1e-40, an ior of 1e+-300 or exactly 1."""
import numpy as np

from rayrs_amd import procedural, scenes
from rayrs_amd.api import Axis, Emission, Fresnel, Material, Object

W, H, SPP, BUDGET = 32, 16, 8, 50
ONE = (1.0, 1.0, 1.0)
F32_TINY = float(np.finfo(np.float32).tiny)        # smallest normal f32
F32_SUB = float(np.float32(1e-40))                  # an f32 subnormal, exact in f64
F32_MAX = float(np.finfo(np.float32).max)


def assert_same_frame_nan_aware(img, ref, what=""):
    """img equals ref where neither is NaN, bit for bit (+0 and -0 still told apart), and the NaN components sit at
    the same places.  The sign and payload of a NaN are NOT compared: x86 makes the negative default NaN, AMDGPU a
    positive canonical one, and the reference (Rust on x86) defines no NaN bits.  Comparisons of the GPU with itself
    in the same kernel stay fully bit-identical instead (np.array_equal on the integer views)."""
    assert img.shape == ref.shape and img.dtype == ref.dtype, (img.shape, ref.shape, img.dtype, ref.dtype)
    ui = np.uint64 if img.dtype == np.float64 else np.uint32
    a, b = np.ascontiguousarray(img), np.ascontiguousarray(ref)
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        bad = (na != nb).reshape(-1, a.shape[-1]).any(axis=1)
        raise AssertionError(f"{what}: NaN components differ in {int(bad.sum())} pixels; first at "
                             f"{np.argwhere((na != nb))[0]}: {a.reshape(-1)[np.flatnonzero(na != nb)[0]]} vs "
                             f"{b.reshape(-1)[np.flatnonzero(na != nb)[0]]}")
    diff = (a.view(ui) != b.view(ui)) & ~na
    if diff.any():
        k = np.flatnonzero(diff)[0]
        raise AssertionError(f"{what}: {int(diff.sum())} non-NaN components differ; first at "
                             f"{np.argwhere(diff)[0]}: {a.reshape(-1)[k]!r} vs {b.reshape(-1)[k]!r}")


def floor_and_sphere(mat, emission=Emission.Dark(), hdri=None, floor_mat=None):
    """single_sphere (test_scenes.rs:14-44) with the given sphere, at W x H."""
    cam_args, objs, heur = scenes.single_sphere(mat)
    objs = list(objs)
    objs[1] = Object.sphere(1.0, (0.0, 1.0, 0.0), mat, emission)
    if floor_mat is not None:
        objs[0] = Object.plane(Axis.Y, -25.0, 25.0, -25.0, 25.0, 0.0, floor_mat, Emission.Dark())
    return scenes.camera_for_resolution(cam_args, W, H), objs, heur, procedural.make_hdri(64, 32) if hdri is None else hdri


def tiny_hdri():
    """Texels of about 1e-40: every one an f32 subnormal."""
    return np.ascontiguousarray((procedural.make_hdri(64, 32) * np.float32(1e-40)).astype(np.float32))


def full_layout(desc):
    """The same scene and a small triangle behind the camera whose vertices are off the f32 grid: the f64 record
    layout (compact == 0)."""
    cam_args, objs, heur, hdri = desc
    objs = list(objs) + [Object.triangle((0.1, 0.1, 30.1), (1.1, 0.1, 30.1), (0.1, 1.1, 30.1),
                                         Material.LambertianDiffuse((0.5, 0.5, 0.5)), Emission.Dark())]
    return cam_args, objs, heur, hdri


# name -> (scene description, what the oracle's frame must show).  Claims: "nan" NaN pixels, "nan_thr" paths whose
# throughput turns NaN and pass the roulette to hit a surface again, "part_nan" pixels NaN in some components only,
# "part_nan_thr" paths whose throughput is NaN in some components only and go on to hit a surface, "inf" infinite
# f64 pixels, "over_f32" finite f64 pixels above FLT_MAX, "sub32" pixels in the f32 subnormal range,
# "big_weight" more than 40 % of the sphere's scattered weights above 1 (the roulette's p > 1 branch), "finite".
FAMILIES = {
    "ct_alpha_1e-200": (lambda: floor_and_sphere(Material.CookTorrance(ONE, 1e-200, Fresnel.SchlickMetallic((0.8, 0.8, 0.8)))),
                        {"nan", "nan_thr"}),
    "ct_alpha_1e-160": (lambda: floor_and_sphere(Material.CookTorrance(ONE, 1e-160, Fresnel.SchlickDielectric(1.45))),
                        {"nan", "nan_thr"}),
    # alpha^2 = 3.0e-309: the Beckmann term near DBL_MAX, so only the colour's blue component overflows, the
    # throughput divided by p = inf becomes (0, 0, NaN), and the next roulette's p ignores that NaN
    "ct_blue_alpha_5.5e-155": (lambda: floor_and_sphere(Material.CookTorrance((0.05, 0.05, 1.0), 5.5e-155,
                                                                              Fresnel.SchlickMetallic((0.9, 0.9, 0.9)))),
                               {"nan", "part_nan_thr"}),
    "ctr_alpha_1e200": (lambda: floor_and_sphere(Material.CookTorranceRefract(ONE, 1e200, 1.45)), {"nan"}),
    "ctg_alpha_1e-200": (lambda: floor_and_sphere(Material.CookTorranceGlass(ONE, 1e-200, 1.45)), {"nan", "nan_thr"}),
    "plastic_alpha_1e-200": (lambda: floor_and_sphere(Material.Plastic((0.7, 0.2, 0.2), ONE, 1e-200, 1.45)),
                             {"nan"}),
    "emit_inf_red": (lambda: floor_and_sphere(Material.LambertianDiffuse((0.8, 0.8, 0.8)),
                                              Emission.new(float("inf"), (1.0, 0.0, 0.0))), {"nan", "part_nan", "inf"}),
    "emit_1e308": (lambda: floor_and_sphere(Material.LambertianDiffuse((0.8, 0.8, 0.8)), Emission.new(1e308, ONE)),
                   {"inf", "over_f32"}),
    "emit_1e-40": (lambda: floor_and_sphere(Material.LambertianDiffuse((0.8, 0.8, 0.8)), Emission.new(1e-40, ONE),
                                            hdri=tiny_hdri()), {"sub32", "finite"}),
    "ctg_ior_1e300": (lambda: floor_and_sphere(Material.CookTorranceGlass((0.9, 1.0, 1.0), 0.15, 1e300)),
                      {"big_weight", "finite"}),
    "plastic_ior_1e-300": (lambda: floor_and_sphere(Material.Plastic((0.7, 0.2, 0.2), ONE, 0.1, 1e-300)),
                           {"big_weight", "finite"}),
    "plastic_ior_1e300": (lambda: floor_and_sphere(Material.Plastic((0.7, 0.2, 0.2), ONE, 0.1, 1e300)),
                          {"big_weight", "finite"}),
    "ctg_ior_1": (lambda: floor_and_sphere(Material.CookTorranceGlass(ONE, 0.1, 1.0)), {"finite"}),
    "glass_ior_1": (lambda: floor_and_sphere(Material.Glass((0.9, 0.9, 0.9), 1.0)), {"finite"}),
}

# the surfaces of the families, plus the other kinds at the same edges: material evaluation on its own
EDGE_MATERIALS = {
    "ct_metal_alpha_1e-200": Material.CookTorrance(ONE, 1e-200, Fresnel.SchlickMetallic((0.8, 0.8, 0.8))),
    "ct_dielectric_alpha_1e-160": Material.CookTorrance(ONE, 1e-160, Fresnel.SchlickDielectric(1.45)),
    "ct_blue_alpha_5.5e-155": Material.CookTorrance((0.05, 0.05, 1.0), 5.5e-155, Fresnel.SchlickMetallic((0.9, 0.9, 0.9))),
    "ct_metal_alpha_1e200": Material.CookTorrance(ONE, 1e200, Fresnel.SchlickMetallic((0.8, 0.8, 0.8))),
    "ctr_alpha_1e200": Material.CookTorranceRefract(ONE, 1e200, 1.45),
    "ctr_alpha_1e-200": Material.CookTorranceRefract(ONE, 1e-200, 1.45),
    "ctg_alpha_1e-200": Material.CookTorranceGlass(ONE, 1e-200, 1.45),
    "ctg_alpha_1e200": Material.CookTorranceGlass(ONE, 1e200, 1.45),
    "plastic_alpha_1e-200": Material.Plastic((0.7, 0.2, 0.2), ONE, 1e-200, 1.45),
    "ctg_ior_1e300": Material.CookTorranceGlass((0.9, 1.0, 1.0), 0.15, 1e300),
    "ctg_ior_1e-300": Material.CookTorranceGlass((0.9, 1.0, 1.0), 0.15, 1e-300),
    "plastic_ior_1e300": Material.Plastic((0.7, 0.2, 0.2), ONE, 0.1, 1e300),
    "plastic_ior_1e-300": Material.Plastic((0.7, 0.2, 0.2), ONE, 0.1, 1e-300),
    "glass_ior_1e300": Material.Glass((0.9, 0.9, 0.9), 1e300),
    "refract_ior_1e-300": Material.Refract((0.9, 0.9, 0.9), 1e-300),
    "ctg_ior_1": Material.CookTorranceGlass(ONE, 0.1, 1.0),
    "ctr_ior_1": Material.CookTorranceRefract(ONE, 0.1, 1.0),
    "glass_ior_1": Material.Glass((0.9, 0.9, 0.9), 1.0),
    "refract_ior_1": Material.Refract((0.9, 0.9, 0.9), 1.0),
    "plastic_ior_1": Material.Plastic((0.7, 0.2, 0.2), ONE, 0.1, 1.0),
}


def edge_normals_views(n=4000, seed=11):
    """The normals and views of test_gpu_functions.py test_material_evaluate_bit_exact."""
    r = np.random.default_rng(seed)

    def unit(v):
        return v / np.sqrt((v * v).sum(axis=1, keepdims=True))
    normal = unit(r.normal(size=(n, 3)))
    view = unit(r.normal(size=(n, 3)))
    view[:50] = normal[:50]
    view[50:100] = unit(view[50:100] - normal[50:100] * (view[50:100] * normal[50:100]).sum(1, keepdims=True))
    normal[100:110] = [0.0, 1.0, 0.0]
    key = r.integers(0, 2 ** 63, n, dtype=np.uint64)
    return np.ascontiguousarray(normal), np.ascontiguousarray(view), key


def odd_hdris():
    """HDRIs of odd shapes (2x2, 3x2, 2x3, 7x5, 1021x3; width x height) whose texels include NaN, +-inf, negative,
    above 3, exactly 3, FLT_MAX and f32-subnormal values, keyed by name."""
    specials = np.array([np.nan, np.inf, -np.inf, -1.5, -F32_SUB, 7.25, 3.0, F32_MAX, F32_SUB, F32_TINY, 2.0 ** -149,
                         0.5, 0.0], dtype=np.float32)
    out = {}
    for k, (w, h) in enumerate(((2, 2), (3, 2), (2, 3), (7, 5), (1021, 3))):
        r = np.random.default_rng(100 + k)
        img = r.uniform(0.0, 3.5, size=(h, w, 3)).astype(np.float32)
        flat = img.reshape(-1)
        pick = r.random(flat.size) < 0.5
        flat[pick] = specials[r.integers(0, len(specials), int(pick.sum()))]
        flat[:len(specials)] = specials[:min(len(specials), flat.size)]
        out[f"{w}x{h}"] = np.ascontiguousarray(img)
    return out


def background_dirs(n=3000, seed=5):
    """Random directions of many magnitudes, plus the poles, the phi seam and directions onto integral texel
    coordinates of a w x h map are added per map by background_dirs_for."""
    r = np.random.default_rng(seed)
    d = r.normal(size=(n, 3)) * 10.0 ** r.uniform(-3, 3, size=(n, 1))
    d[:6] = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
    d[6] = [-1.0, 0.0, -1e-300]
    d[7] = [-1.0, 0.0, 1e-300]
    d[8] = [-1.0, 0.0, 0.0]
    return d


def background_dirs_for(w, h, n=3000, seed=5):
    d = list(background_dirs(n, seed))
    # directions whose texel coordinates x = phi / 2pi * (w - 1), y = theta / pi * (h - 1) are integers
    for j in range(min(w, 12)):
        for i in range(h):
            phi = j / (w - 1) * 2.0 * np.pi - np.pi
            theta = i / (h - 1) * np.pi
            d.append([np.sin(theta) * np.cos(phi), np.cos(theta), np.sin(theta) * np.sin(phi)])
    return np.ascontiguousarray(np.array(d, dtype=np.float64))


def subnormal_coordinate_scene():
    """A triangle and a sphere whose f32-exact coordinates include f32 subnormals: still the compact layout."""
    s = F32_SUB
    tri = [Object.triangle((-2.0, s, -2.0), (2.0, s, -2.0), (0.0, 2.0 * s, 2.0),
                           Material.LambertianDiffuse((0.8, 0.8, 0.8)), Emission.Dark()),
           Object.triangle((-2.0, 0.5, s), (2.0, 0.5, -s), (s, 3.0, 0.0),
                           Material.CookTorrance(ONE, 0.2, Fresnel.SchlickMetallic((0.9, 0.6, 0.3))), Emission.Dark()),
           Object.sphere(0.5, (1.5, 0.5 + 2.0 ** -20, 0.0), Material.Glass((0.9, 0.9, 0.9), 1.5), Emission.new(0.5, ONE))]
    cam_args, _, heur = scenes.single_sphere(Material.NoReflect())
    return scenes.camera_for_resolution(cam_args, W, H), tri, heur, procedural.make_hdri(64, 32)
