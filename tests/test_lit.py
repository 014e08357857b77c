"""Light sampling (include/rayrs_hip.h LIGHT SAMPLING) without a GPU: the entry points are declared, exported and bound, every
refusal that is decided before the device is touched comes in the header's order, the kernels keep their resources -- and the
plain-Python reading of the operation (tests/_lit.py) is held to what makes it a reading worth comparing with: without lights it
is the oracle's radiance(), its densities are the densities of the directions it generates, and with lights its irradiance has
the unlit mean and less variance."""
import os
import re

import numpy as np
import pytest

import _ao
import _geometry_reading as G
import _lit
import _oracle
import rayrs_amd
from rayrs_amd import _ffi, procedural, scenes
from rayrs_amd.api import Axis, Emission, Fresnel, Material, Object
from test_features import HIPCC, compile_asm, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["rayrs_scene_radiance_lit", "rayrs_scene_radiance_lit_launch", "rayrs_scene_irradiance_lit",
               "rayrs_scene_irradiance_lit_launch", "rayrs_render_lit"]
INVALID_ARG, NO_DEVICE, UNSUPPORTED = -1, -4, -5
HDRI = procedural.make_hdri(128, 64)
Z_NEAR, Z_FAR = 1e-6, 1e6
F = np.float64


def header():
    return open(os.path.join(ROOT, "include", "rayrs_hip.h")).read()


def test_the_header_declares_the_entry_points_with_their_contract():
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\bint {name}\s*\(", code), name
    assert re.search(r"#define RAYRS_MAX_LIGHTS 8\b", code)
    text = re.sub(r"\s+", " ", re.sub(r"\s*\n \*\s*", " ", header()))
    assert "LIGHT SAMPLING, specified to the operation" in text
    assert "b = rng.next(); k = min((uint32)(b * (double)K), K - 1)" in text
    assert "l = (q - position).unit()" in text
    assert "pdf = +inf if ndl < 0.0" in text
    assert "else 0.5 * p_L + 0.5 * (ndl * RR_FRAC_1_PI)" in text
    assert "p_L = (p_0 assigned, then += p_k in list order) / (double)K" in text
    assert "color = ((albedo * RR_FRAC_1_PI) * ndl) / pdf" in text
    assert "p_k(l) is the TRUE solid-angle density" in text and "deliberately leaves the reference" in text
    assert "|n_k . l| * area" in text and "if t1 > 0.0: p_k = p_k + X(t1); if t2 > 0.0: p_k = p_k + X(t2)" in text
    assert "L_{i,s} = color * radiance(scene, Ray{position, l}, max_bounces)" in text
    assert "`lights` is a HOST pointer in every form" in text
    assert text.index("RADIANCE QUERY, specified") < text.index("LIGHT SAMPLING, specified")
    assert int(re.search(r"#define RAYRS_ABI_VERSION (\d+)", header()).group(1)) == 7


def test_the_binding_declares_and_the_library_exports_the_entry_points():
    L = _ffi.lib()
    assert L.rayrs_abi_version() == _ffi.ABI_VERSION == 7
    for name in NEW_SYMBOLS:
        assert name in _ffi.SYMBOLS and hasattr(L, name) and getattr(L, name).argtypes, name
    for name in ("render_lit", "emitters"):
        assert hasattr(rayrs_amd, name) and name in rayrs_amd.__all__, name
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"fn {name}\(", text), name


def test_emitters_numbers_objects_as_the_scene_does():
    cam_args, objs, heur = scenes.mesh_scene(1, Material.LambertianDiffuse((0.8, 0.8, 0.8)), area_light=True)
    n_tri = sum(int(o.idx.shape[0]) for o in rayrs_amd.api.flatten_objects(objs) if o.kind == "mesh")
    assert n_tri == 80 and rayrs_amd.emitters(objs) == [1 + n_tri]
    cam, room, heur, names = _lit.lit_room()
    assert rayrs_amd.emitters(room) == [names["sphere_lamp"], names["rect_lamp"]]
    tri = Object.triangle((0, 0, 0), (1, 0, 0), (0, 1, 0), Material.LambertianDiffuse((1, 1, 1)), Emission.new(1.0, (1, 1, 1)))
    assert rayrs_amd.emitters([tri, [room]]) == [1 + names["sphere_lamp"], 1 + names["rect_lamp"]]   # (no triangle lights)


def host_scene():
    cam, objs, heur, names = _lit.lit_room()
    objs = objs + [Object.triangle((0, 0, 0), (1, 0, 0), (0, 1, 0), Material.NoReflect(), Emission.Dark())]
    return rayrs_amd.Scene(objs, Z_NEAR, Z_FAR, heur, HDRI, device=-1), len(objs) - 1


@pytest.mark.parametrize("n", [4, 0])
def test_refusals_on_a_host_only_scene_come_in_the_headers_order(n):
    """RADIANCE QUERY's order with the list's refusals in their groups: RAYRS_INVALID_ARG (also lights == NULL with n_lights > 0,
    an index >= the object count) whatever else is wrong beside it, then RAYRS_UNSUPPORTED (also n_lights > 8, an index that
    names a triangle), and only then RAYRS_NO_DEVICE."""
    L = _ffi.lib()
    scene, tri = host_scene()
    a, b = np.zeros((4, 3)), np.ones((4, 3))
    rad, cnt = np.zeros((4, 3)), np.zeros(4, dtype=np.uint32)
    P = lambda x: x.ctypes.data
    good = np.array([3, 4, 5], dtype=np.uint32)

    def call(irr, launch, scene_h=scene._h, a_=P(a), b_=P(b), samples=4, bounces=50, chunk=0, fast=0, lights=good, n_lights=None, rad_=P(rad),
             cnt_=P(cnt)):
        lp = None if lights is None else P(lights)
        nl = (0 if lights is None else len(lights)) if n_lights is None else n_lights
        args = (scene_h, a_, b_, n, samples, bounces, chunk) + ((1e-4,) if irr else ()) + (1, 0, fast, lp, nl, rad_, cnt_)
        name = "rayrs_scene_irradiance_lit" if irr else "rayrs_scene_radiance_lit"
        return getattr(L, name + "_launch")(*args, None) if launch else getattr(L, name)(*args)

    u32 = lambda *v: np.array(v, dtype=np.uint32)
    nine = u32(3, 4, 5, 3, 4, 5, 3, 4, 5)
    for irr in (False, True):
        for launch in (False, True):
            for bad in (dict(scene_h=None), dict(a_=None), dict(b_=None), dict(rad_=None, cnt_=None), dict(samples=0), dict(fast=2),
                        dict(lights=None, n_lights=3), dict(lights=u32(3, tri + 1)), dict(lights=u32(0xffffffff)),
                        dict(lights=u32(3, 4, 5, 3, 4, 5, 3, 4, tri + 1))):
                assert call(irr, launch, **bad) == INVALID_ARG, (irr, launch, bad)
                if "samples" not in bad:
                    assert call(irr, launch, bounces=8001, **bad) == INVALID_ARG
                    assert call(irr, launch, samples=1 << 30, **bad) == INVALID_ARG
            for big in (dict(samples=1 << 30), dict(bounces=8001), dict(samples=1 << 20, bounces=4096), dict(samples=(1 << 21) + 1, chunk=1, bounces=1),
                        dict(lights=nine), dict(lights=u32(3, tri)), dict(lights=u32(tri))):
                assert call(irr, launch, **big) == UNSUPPORTED, (irr, launch, big)
            for ok in (dict(), dict(fast=1), dict(rad_=None), dict(cnt_=None), dict(bounces=0), dict(lights=None), dict(lights=u32(), n_lights=0),
                       dict(lights=u32(3, 3, 3, 3, 4, 4, 4, 4)), dict(lights=u32(0, 1, 2)), dict(samples=1 << 20, chunk=1, bounces=4095)):
                assert call(irr, launch, **ok) == NO_DEVICE, (irr, launch, ok)
    # the image form
    cam = rayrs_amd.Camera(*scenes.camera_for_resolution(_lit.lit_room()[0], 16, 8))
    img = np.zeros((8, 16, 3))
    import ctypes as C

    def render(scene_h=scene._h, cam_=C.byref(cam.desc), samples=4, bounces=50, fast=0, lights=good, out=P(img), cnt_=None):
        return L.rayrs_render_lit(scene_h, cam_, 1, samples, bounces, 0, fast, None if lights is None else P(lights), 0 if lights is None else len(lights),
                                  out, cnt_)
    for bad in (dict(scene_h=None), dict(cam_=None), dict(out=None), dict(samples=0), dict(fast=2), dict(lights=u32(tri + 1))):
        assert render(**bad) == INVALID_ARG, bad
        assert render(bounces=8001, **bad) == INVALID_ARG, bad
    for big in (dict(bounces=8001), dict(lights=nine), dict(lights=u32(tri))):
        assert render(**big) == UNSUPPORTED, big
    for ok in (dict(), dict(lights=None), dict(fast=1)):
        assert render(**ok) == NO_DEVICE, ok
    if n:
        for f in (scene.radiance, scene.irradiance):
            with pytest.raises(_ffi.RayrsError) as e:
                f(a, b, lights=[3, 4])
            assert e.value.status == NO_DEVICE
            with pytest.raises(_ffi.RayrsError) as e:
                f(a, b, lights=[tri])
            assert e.value.status == UNSUPPORTED
            with pytest.raises(ValueError):
                f(a, b, lights=[-1])
            with pytest.raises(ValueError):
                f(np.zeros((4, 2)), b, lights=[3])


# ---- kernel resources: what radiance_kernel is held to (tests/test_radiance.py)
VGPR_BOUND = 256


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_the_lit_kernels_use_no_scratch_and_keep_two_waves_per_simd(tmp_path):
    res = kernel_resources(compile_asm("radiance_lit.hip", tmp_path))
    path = {n: r for n, r in res.items() if "radiance_lit_kernel" in n}
    resolve = {n: r for n, r in res.items() if "radiance_lit_resolve_kernel" in n}
    assert len(path) == 12 and len(resolve) == 1 and len(res) == 13   # COMPACT x EXACT x the three starts; the resolve
    for name, (vgpr, scratch, lds) in res.items():
        assert vgpr <= VGPR_BOUND and scratch == 0 and lds == 0, (name, vgpr, scratch, lds)   # (the stacks are dynamic LDS)


# ---- the reading is sound

def nine_materials():
    mats = [Material.LambertianDiffuse((0.8, 0.7, 0.6)), Material.Plastic((0.8, 0.8, 0.8), (1, 1, 1), 0.05, 1.45), Material.Reflect((0.8, 0.8, 0.8)),
            Material.Refract((0.9, 0.9, 0.9), 1.3), Material.CookTorrance((1, 1, 1), 0.05, Fresnel.SchlickMetallic((0.8, 0.8, 0.8))),
            Material.Glass((1, 1, 1), 1.45), Material.CookTorranceRefract((1, 1, 1), 0.1, 1.45), Material.CookTorranceGlass((1, 1, 1), 0.05, 1.45),
            Material.NoReflect()]
    cam = ((0.0, 3.0, 24.0), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), 90.0, 1920.0 / 500.0, 250.0 / 500.0, 125)
    return scenes.multiple_spheres(mats, cam)


@pytest.mark.parametrize("name", ["material_test", "mesh3_light", "nine_materials"])
def test_without_lights_the_reading_is_the_oracles_radiance(name):
    make, w, h = {"material_test": (scenes.material_test, 48, 10), "nine_materials": (nine_materials, 60, 8),
                  "mesh3_light": (lambda: scenes.mesh_scene(3, Material.LambertianDiffuse((0.8, 0.8, 0.8)), area_light=True), 32, 24)}[name]
    cam_args, objs, heur = make()
    R = _lit.Reading(objs, Z_NEAR, Z_FAR, heur, HDRI)
    ocam = _oracle.OracleCamera(*scenes.camera_for_resolution(cam_args, w, h))
    kinds, deep = set(), 0
    for r in range(h):
        for c in range(w):
            o, d, _ = ocam.primary_ray(h - r, w - c, _ao.path_key(77, r * w + c, 0))
            first = R.osc.intersect(o, d, Z_NEAR, Z_FAR)[0]
            if first >= 0:
                kinds.add(R.prims.list[first].mat.kind)
            for s in range(2):
                key = _ao.path_key(0x5EED, r * w + c, s)
                got, want = R.path(o, d, 50, key, 0, []), R.osc.radiance(o, d, 50, key, 0)
                assert got[0].tobytes() == want[0].tobytes() and got[1:] == want[1:], (name, r, c, s, got, want)
                deep += got[1] >= 4
    print(name, "material kinds at first hits", sorted(kinds), "paths of four queries and more", deep)
    assert deep >= 10
    if name == "nine_materials":
        assert kinds == set(range(9))


# ---- the densities are densities: E[1 / p_k(l)] over generated l is the solid angle of what the arm can reach

def lamp_scene():
    objs = [Object.sphere(0.25, (0.0, 2.5, 0.0), Material.NoReflect(), Emission.Dark()),
            Object.plane(Axis.YRev, 1.0, 2.0, -2.0, -1.0, 3.5, Material.NoReflect(), Emission.Dark())]
    return _lit.Reading(objs, Z_NEAR, Z_FAR, ("sah", 1000), HDRI)


def mean_inverse_density(R, k, position, n, seed, **kw):
    rng = np.random.default_rng(seed)
    u = rng.random((n, 2))
    inv = np.zeros(n)
    with np.errstate(all="ignore"):
        for i in range(n):
            l = G.unit(G.sub(R.light_sample(k, F(u[i, 0]), F(u[i, 1])), position))
            inv[i] = F(1.0) / R.light_density(k, position, l, **kw)
    return inv.mean(), inv.std(ddof=1) / np.sqrt(n)


def test_the_densities_are_densities():
    R = lamp_scene()
    n = 4000
    # a sphere seen from outside: 2 pi (1 - cos theta_max), sin theta_max = r / distance
    position = _lit.f3((0.3, 0.0, 0.4))
    dist2 = 0.3 ** 2 + 2.5 ** 2 + 0.4 ** 2
    omega = 2.0 * np.pi * (1.0 - np.sqrt(1.0 - 0.25 ** 2 / dist2))
    mean, se = mean_inverse_density(R, 0, position, n, 1)
    print("sphere from outside: solid angle", omega, "mean 1/p", mean, "+-", se)
    assert abs(mean - omega) <= 4.0 * se
    near, near_se = mean_inverse_density(R, 0, position, n, 1, near_root_only=True)
    print("  the near root alone (the reference's reading):", near, "+-", near_se)
    assert abs(near - omega) > 4.0 * near_se and near > 1.5 * omega   # no density: it prices half of what is sampled
    # from inside: every direction, 4 pi
    mean, se = mean_inverse_density(R, 0, _lit.f3((0.05, 2.45, -0.1)), n, 2)
    print("sphere from inside: 4 pi", 4.0 * np.pi, "mean 1/p", mean, "+-", se)
    assert abs(mean - 4.0 * np.pi) <= 4.0 * se
    # a rectangle, one unit below it and off its centre: the share of uniform directions that hit it, times 4 pi
    position = _lit.f3((1.2, 2.5, -1.3))
    mean, se = mean_inverse_density(R, 1, position, n, 3)
    m = 400000
    rng = np.random.default_rng(4)
    z = 1.0 - 2.0 * rng.random(m)
    phi = 2.0 * np.pi * rng.random(m)
    s = np.sqrt(1.0 - z * z)
    d = (s * np.cos(phi), z, s * np.sin(phi))
    with np.errstate(all="ignore"):
        some, t = G.plane_intersect(int(Axis.YRev), 1.0, 2.0, -2.0, -1.0, 3.5, tuple(np.full(m, x) for x in position), d)
    hit = some & (t > 0.0)
    share = hit.mean()
    omega, omega_se = 4.0 * np.pi * share, 4.0 * np.pi * np.sqrt(share * (1.0 - share) / m)
    print("rectangle: solid angle", omega, "+-", omega_se, "mean 1/p", mean, "+-", se)
    assert hit.sum() >= 10000 and abs(mean - omega) <= 4.0 * np.hypot(se, omega_se)


# ---- unbiased, and less noise

def test_lit_irradiance_has_the_unlit_mean_and_less_variance():
    """The small room (sphere lamp, rectangle lamp), three floor points, fixed seeds: the reading's lit and unlit means agree
    within 4 combined standard errors in every channel, and the lit variance is the lower one.  A sample is a vector, and its
    variance here is the sum of the three channels' (what scripts/ubench/lit_bench.py reports per ray).  Channel by channel the
    inequality is not the operation's promise: the mix spends half of its directions on the lamps, so a channel whose noise
    comes from the environment -- blue, at the far corner, where the lamps are small and low -- gets up to twice the
    cosine lobe's variance (1.49 times there); the ratios are printed per channel."""
    cam, objs, heur, names = _lit.lit_room()
    R = _lit.Reading(objs, Z_NEAR, Z_FAR, heur, HDRI)
    points = np.array([(0.0, 0.0, 0.0), (1.5, 0.0, -1.5), (-3.0, 0.0, 3.0)])
    normals = np.tile((0.0, 1.0, 0.0), (len(points), 1))
    lights = [names["sphere_lamp"], names["rect_lamp"]]
    assert lights == rayrs_amd.emitters(objs)
    s_lit, s_unlit = 2000, 8000
    lit, _ = _lit.irradiance_paths(R, points, normals, s_lit, 1e-4, 50, 11, lights)
    unlit, _ = _lit.irradiance_paths(R, points, normals, s_unlit, 1e-4, 50, 12, [])
    assert np.isfinite(lit).all() and np.isfinite(unlit).all()
    for i in range(len(points)):
        ml, mu = lit[i].mean(axis=0), unlit[i].mean(axis=0)
        vl, vu = lit[i].var(axis=0, ddof=1), unlit[i].var(axis=0, ddof=1)
        se = np.sqrt(vl / s_lit + vu / s_unlit)
        print("point", points[i].tolist(), "lit", ml, "unlit", mu, "difference / se", (ml - mu) / se, "variance lit / unlit", vl / vu)
        assert (np.abs(ml - mu) <= 4.0 * se).all(), (i, ml, mu, se)
        assert vl.sum() < vu.sum(), (i, vl, vu)
