"""Direct lighting (include/rayrs_hip.h DIRECT LIGHTING) without a GPU: the header states the operation, the entry points are
declared, exported and bound, every refusal that is decided before the device is touched comes in the header's order -- the
material rule and the wider overflow guard among them --, the kernels keep their resources, and the plain-Python reading of the
operation (tests/_direct.py) is held to what makes it a reading worth comparing with: without lights it is the oracle's
radiance(), with lights its irradiance has the unlit mean, it is finite where the mix of LIGHT SAMPLING is not, and the paths the
tests walk take every branch of the turn."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import _ao
import _direct
import _lit
import _oracle
import rayrs_amd
from rayrs_amd import _ffi, procedural, scenes
from rayrs_amd.api import Emission, Material, Object
from test_features import HIPCC, compile_asm, kernel_resources
from test_lit import nine_materials

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["rayrs_scene_radiance_direct", "rayrs_scene_radiance_direct_launch", "rayrs_scene_irradiance_direct",
               "rayrs_scene_irradiance_direct_launch", "rayrs_render_direct"]
INVALID_ARG, NO_DEVICE, UNSUPPORTED = -1, -4, -5
HDRI = procedural.make_hdri(128, 64)
Z_NEAR, Z_FAR = 1e-6, 1e6
F = np.float64


def header():
    return open(os.path.join(ROOT, "include", "rayrs_hip.h")).read()


def test_the_header_states_the_operation():
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\bint {name}\s*\(", code), name
    text = re.sub(r"\s+", " ", re.sub(r"\s*\n \*\s*", " ", header()))
    assert "DIRECT LIGHTING, specified to the operation" in text
    assert text.index("LIGHT SAMPLING, specified") < text.index("DIRECT LIGHTING, specified")
    assert "w = 1.0 at a path's start, and w = 1.0 after every bounce that is not a diffuse bounce" in text
    assert "ev = Material::evaluate(position, normal, view, None)" in text
    assert "e = obj.emission.emit(); if obj is in the list: e = e * w" in text
    assert "light = light + throughput * e" in text
    assert "b = rng.next(); u1 = rng.next(); u2 = rng.next()" in text
    assert "k = min((uint32)(b * (double)K), K - 1); q = light k's Hittable::sample(u1, u2); l_s = (q - position).unit()" in text
    assert "if ndl_s > 0.0: den = p_L(position, l_s) + ndl_s * RR_FRAC_1_PI" in text
    assert "if den < +inf:" in text
    assert "C = ((albedo * RR_FRAC_1_PI) * ndl_s) / den" in text
    assert "hit_s = Bvh::intersect(Ray{position, l_s}, z_near, z_far)" in text
    assert "light = light + (throughput * C) * hit_s.obj.emission.emit()" in text
    assert "pc = ndl * RR_FRAC_1_PI; pl = p_L(position, l)" in text
    assert "w_next = pc / (pc + pl) if pl > 0.0 else 1.0" in text
    assert "credited BEFORE the roulette" in text and "does not count against max_bounces" in text
    assert "Why it is unbiased" in text and "The two weights sum to 1 wherever a listed object is the first thing seen" in text
    assert "LambertianDiffuse, Reflect or Glass" in text and "A dark listed object (a portal) may have any material" in text
    assert "L_{i,s} = credit + radiance(scene, Ray{position, l}, max_bounces)" in text and "the path going on at draw 5" in text
    assert "(uint64)samples * (2 * max_bounces + 1) >= 2^32" in text
    assert int(re.search(r"#define RAYRS_ABI_VERSION (\d+)", header()).group(1)) == 7
    assert "rayrs_render_direct (DIRECT LIGHTING)" in text   # (the version comment)


def test_the_binding_declares_and_the_library_exports_the_entry_points():
    L = _ffi.lib()
    assert L.rayrs_abi_version() == _ffi.ABI_VERSION == 7
    for name in NEW_SYMBOLS:
        lit = name.replace("_direct", "_lit")
        assert name in _ffi.SYMBOLS and hasattr(L, name) and getattr(L, name).argtypes == getattr(L, lit).argtypes, name
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"fn {name}\(", text), name


def test_direct_is_the_last_keyword_of_the_three_calls_and_needs_a_list():
    for f in (rayrs_amd.Scene.radiance, rayrs_amd.Scene.irradiance, rayrs_amd.render_lit):
        last = list(inspect.signature(f).parameters.values())[-1]
        assert last.name == "direct" and last.default is False, f
    scene, _ = host_scene()
    a, b = np.zeros((4, 3)), np.ones((4, 3))
    for f in (scene.radiance, scene.irradiance):
        with pytest.raises(ValueError):
            f(a, b, direct=True)
        with pytest.raises(_ffi.RayrsError) as e:
            f(a, b, lights=[3, 4], direct=True)
        assert e.value.status == NO_DEVICE
        with pytest.raises(_ffi.RayrsError) as e:
            f(a, b, lights=[scene_names["plastic_lamp"]], direct=True)
        assert e.value.status == UNSUPPORTED
        with pytest.raises(_ffi.RayrsError) as e:   # (LIGHT SAMPLING has no material rule)
            f(a, b, lights=[scene_names["plastic_lamp"]])
        assert e.value.status == NO_DEVICE
    cam = rayrs_amd.Camera(*scenes.camera_for_resolution(_lit.lit_room()[0], 16, 8))
    with pytest.raises(ValueError):
        rayrs_amd.render_lit(scene, cam, 2, None, direct=True)
    with pytest.raises(_ffi.RayrsError) as e:
        rayrs_amd.render_lit(scene, cam, 2, [3], direct=True)
    assert e.value.status == NO_DEVICE


scene_names = {}


def host_scene():
    """tests/test_lit.py's host-only room and its triangle, and after them three spheres for the material rule: an emitting
    Plastic one, an emitting NoReflect one, a dark Plastic one; and emitting Refract and Glass ones."""
    cam, objs, heur, names = _lit.lit_room()
    objs = objs + [Object.triangle((0, 0, 0), (1, 0, 0), (0, 1, 0), Material.NoReflect(), Emission.Dark())]
    tri = len(objs) - 1
    glow = Emission.new(5.0, (1.0, 1.0, 1.0))
    plastic = Material.Plastic((0.7, 0.2, 0.2), (1.0, 1.0, 1.0), 0.2, 1.5)
    extra = [("plastic_lamp", plastic, glow), ("noreflect_lamp", Material.NoReflect(), glow), ("plastic_dark", plastic, Emission.Dark()),
             ("refract_lamp", Material.Refract((0.9, 0.9, 0.9), 1.3), glow), ("glass_lamp", Material.Glass((1, 1, 1), 1.45), glow),
             ("noreflect_dark", Material.NoReflect(), Emission.Dark())]
    for i, (name, mat, em) in enumerate(extra):
        scene_names[name] = len(objs)
        objs.append(Object.sphere(0.1, (3.0, 0.2, -3.0 + 0.5 * i), mat, em))
    return rayrs_amd.Scene(objs, Z_NEAR, Z_FAR, heur, HDRI, device=-1), tri


@pytest.mark.parametrize("n", [4, 0])
def test_refusals_on_a_host_only_scene_come_in_the_headers_order(n):
    """LIGHT SAMPLING's refusals in its order (tests/test_lit.py), with the material rule in the RAYRS_UNSUPPORTED group -- a
    listed emitting Plastic, NoReflect or Refract sphere; the same Plastic sphere dark is accepted, and so is an emitting Glass
    one -- and the overflow guard at (uint64)samples * (2 * max_bounces + 1) >= 2^32."""
    L = _ffi.lib()
    scene, tri = host_scene()
    N = scene_names
    a, b = np.zeros((4, 3)), np.ones((4, 3))
    rad, cnt = np.zeros((4, 3)), np.zeros(4, dtype=np.uint32)
    P = lambda x: x.ctypes.data
    good = np.array([3, 4, 5], dtype=np.uint32)

    def call(irr, launch, scene_h=scene._h, a_=P(a), b_=P(b), samples=4, bounces=50, chunk=0, fast=0, lights=good, n_lights=None, rad_=P(rad),
             cnt_=P(cnt)):
        lp = None if lights is None else P(lights)
        nl = (0 if lights is None else len(lights)) if n_lights is None else n_lights
        args = (scene_h, a_, b_, n, samples, bounces, chunk) + ((1e-4,) if irr else ()) + (1, 0, fast, lp, nl, rad_, cnt_)
        name = "rayrs_scene_irradiance_direct" if irr else "rayrs_scene_radiance_direct"
        return getattr(L, name + "_launch")(*args, None) if launch else getattr(L, name)(*args)

    u32 = lambda *v: np.array(v, dtype=np.uint32)
    nine = u32(3, 4, 5, 3, 4, 5, 3, 4, 5)
    for irr in (False, True):
        for launch in (False, True):
            for bad in (dict(scene_h=None), dict(a_=None), dict(b_=None), dict(rad_=None, cnt_=None), dict(samples=0), dict(fast=2),
                        dict(lights=None, n_lights=3), dict(lights=u32(3, 100)), dict(lights=u32(0xffffffff)),
                        dict(lights=u32(N["plastic_lamp"], 100))):
                assert call(irr, launch, **bad) == INVALID_ARG, (irr, launch, bad)
                if "samples" not in bad:
                    assert call(irr, launch, bounces=8001, **bad) == INVALID_ARG
                    assert call(irr, launch, samples=1 << 30, **bad) == INVALID_ARG
            for big in (dict(samples=1 << 30), dict(bounces=8001), dict(samples=1 << 20, bounces=2048), dict(samples=(1 << 21) + 1, chunk=1, bounces=1),
                        dict(samples=(1 << 30) - 1, bounces=2, chunk=1 << 12),   # (2^30 - 1) * 5 >= 2^32, where * 2 is not
                        dict(lights=nine), dict(lights=u32(3, tri)), dict(lights=u32(tri)),
                        dict(lights=u32(N["plastic_lamp"])), dict(lights=u32(N["noreflect_lamp"])), dict(lights=u32(N["refract_lamp"])),
                        dict(lights=u32(3, 4, N["plastic_lamp"], 5))):
                assert call(irr, launch, **big) == UNSUPPORTED, (irr, launch, big)
            for ok in (dict(), dict(fast=1), dict(rad_=None), dict(cnt_=None), dict(bounces=0), dict(lights=None), dict(lights=u32(), n_lights=0),
                       dict(lights=u32(3, 3, 3, 3, 4, 4, 4, 4)), dict(lights=u32(0, 1, 2)), dict(samples=1 << 20, chunk=1, bounces=2047),
                       dict(lights=u32(N["plastic_dark"])), dict(lights=u32(N["noreflect_dark"], 3)), dict(lights=u32(N["glass_lamp"]))):
                assert call(irr, launch, **ok) == NO_DEVICE, (irr, launch, ok)
    # the image form
    cam = rayrs_amd.Camera(*scenes.camera_for_resolution(_lit.lit_room()[0], 16, 8))
    img = np.zeros((8, 16, 3))

    def render(scene_h=scene._h, cam_=C.byref(cam.desc), samples=4, bounces=50, fast=0, lights=good, out=P(img), cnt_=None):
        return L.rayrs_render_direct(scene_h, cam_, 1, samples, bounces, 0, fast, None if lights is None else P(lights),
                                     0 if lights is None else len(lights), out, cnt_)
    for bad in (dict(scene_h=None), dict(cam_=None), dict(out=None), dict(samples=0), dict(fast=2), dict(lights=u32(100))):
        assert render(**bad) == INVALID_ARG, bad
        assert render(bounces=8001, **bad) == INVALID_ARG, bad
    for big in (dict(bounces=8001), dict(lights=nine), dict(lights=u32(tri)), dict(lights=u32(N["plastic_lamp"])),
                dict(lights=u32(N["noreflect_lamp"])), dict(samples=1 << 20, bounces=2048)):
        assert render(**big) == UNSUPPORTED, big
    for ok in (dict(), dict(lights=None), dict(fast=1), dict(lights=u32(N["plastic_dark"])), dict(samples=1 << 20, bounces=2047)):
        assert render(**ok) == NO_DEVICE, ok


# ---- kernel resources: what the lit kernels are held to (tests/test_lit.py)
VGPR_BOUND = 256


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_the_direct_kernels_use_no_scratch_and_keep_two_waves_per_simd(tmp_path):
    res = kernel_resources(compile_asm("radiance_direct.hip", tmp_path))
    path = {n: r for n, r in res.items() if "radiance_direct_kernel" in n}
    resolve = {n: r for n, r in res.items() if "radiance_direct_resolve_kernel" in n}
    assert len(path) == 12 and len(resolve) == 1 and len(res) == 13   # COMPACT x EXACT x the three starts; the resolve
    for name, (vgpr, scratch, lds) in res.items():
        print(name, vgpr, scratch, lds)
        assert vgpr <= VGPR_BOUND and scratch == 0 and lds == 0, (name, vgpr, scratch, lds)   # (the stacks are dynamic LDS)


# ---- the reading is sound

@pytest.mark.parametrize("name", ["material_test", "mesh3_light", "nine_materials"])
def test_without_lights_the_reading_is_the_oracles_radiance(name):
    make, w, h = {"material_test": (scenes.material_test, 48, 10), "nine_materials": (nine_materials, 60, 8),
                  "mesh3_light": (lambda: scenes.mesh_scene(3, Material.LambertianDiffuse((0.8, 0.8, 0.8)), area_light=True), 32, 24)}[name]
    cam_args, objs, heur = make()
    R = _direct.Reading(objs, Z_NEAR, Z_FAR, heur, HDRI)
    ocam = _oracle.OracleCamera(*scenes.camera_for_resolution(cam_args, w, h))
    deep = 0
    for r in range(h):
        for c in range(w):
            o, d, _ = ocam.primary_ray(h - r, w - c, _ao.path_key(77, r * w + c, 0))
            for s in range(2):
                key = _ao.path_key(0x5EED, r * w + c, s)
                got, want = R.path(o, d, 50, key, 0, []), R.osc.radiance(o, d, 50, key, 0)
                assert got[0].tobytes() == want[0].tobytes() and got[1:] == want[1:], (name, r, c, s, got, want)
                deep += got[1] >= 4
    print(name, "paths of four queries and more", deep)
    assert deep >= 10
    # the point form without lights is IRRADIANCE: tests/_lit.py's reading of it, draw for draw
    pts = np.array([(0.3 * i - 2.0, 0.0, 0.2 * i - 1.0) for i in range(12)])
    nrm = np.tile((0.0, 1.0, 0.0), (len(pts), 1))
    a = _direct.irradiance_paths(R, pts, nrm, 3, 1e-4, 50, 5, [])
    b = _lit.irradiance_paths(_lit.Reading(objs, Z_NEAR, Z_FAR, heur, HDRI, osc=R.osc), pts, nrm, 3, 1e-4, 50, 5, [])
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])


# ---- unbiased

def test_direct_irradiance_has_the_unlit_mean():
    """tests/test_lit.py's room, points, sample counts, seeds and margin: the reading's direct and unlit means agree within 4
    combined standard errors in every channel.  The per-channel variance ratios direct / unlit and lit / unlit are printed, not
    asserted on."""
    cam, objs, heur, names = _lit.lit_room()
    R = _direct.Reading(objs, Z_NEAR, Z_FAR, heur, HDRI)
    points = np.array([(0.0, 0.0, 0.0), (1.5, 0.0, -1.5), (-3.0, 0.0, 3.0)])
    normals = np.tile((0.0, 1.0, 0.0), (len(points), 1))
    lights = [names["sphere_lamp"], names["rect_lamp"]]
    assert lights == rayrs_amd.emitters(objs)
    s_direct, s_unlit = 2000, 8000
    direct, dq = _direct.irradiance_paths(R, points, normals, s_direct, 1e-4, 50, 11, lights)
    lit, _ = _lit.irradiance_paths(_lit.Reading(objs, Z_NEAR, Z_FAR, heur, HDRI, osc=R.osc), points, normals, s_direct, 1e-4, 50, 11, lights)
    unlit, uq = _direct.irradiance_paths(R, points, normals, s_unlit, 1e-4, 50, 12, [])
    assert np.isfinite(direct).all() and np.isfinite(unlit).all()
    for i in range(len(points)):
        md, mu = direct[i].mean(axis=0), unlit[i].mean(axis=0)
        vd, vl, vu = direct[i].var(axis=0, ddof=1), lit[i].var(axis=0, ddof=1), unlit[i].var(axis=0, ddof=1)
        se = np.sqrt(vd / s_direct + vu / s_unlit)
        print("point", points[i].tolist(), "direct", md, "unlit", mu, "difference / se", (md - mu) / se, "variance direct / unlit", vd / vu,
              "lit / unlit", vl / vu, "queries per path direct", dq[i].mean(), "unlit", uq[i].mean())
        assert (np.abs(md - mu) <= 4.0 * se).all(), (i, md, mu, se)


# ---- finite where the mix is not

LIT_NAN_SAMPLES = 113   # of 64 * 4, counted on the CPU: the lit reading's samples with a NaN on _direct.lamp_rays(), seed 3


def test_direct_is_finite_where_the_mix_makes_nan():
    """The level-1 mesh scene's lamp is a Lambertian rectangle, and it is the list.  A path that scatters on it under LIGHT
    SAMPLING draws the lamp itself half of the time: l lies in the lamp's plane, ndl = 0, pdf = 0 and the colour is 0 / 0.  The
    same draw under DIRECT LIGHTING is a shadow sample with ndl_s = 0, which is skipped."""
    cam_args, objs, heur = scenes.mesh_scene(1, Material.LambertianDiffuse((0.8, 0.8, 0.8)), area_light=True)
    lights = rayrs_amd.emitters(objs)
    assert len(lights) == 1 and objs[-1].mat.kind == rayrs_amd.api.MAT_LAMBERTIAN
    R = _direct.Reading(objs, Z_NEAR, Z_FAR, heur, HDRI)
    o, d = _direct.lamp_rays()
    lit, _ = _lit.radiance_paths(_lit.Reading(objs, Z_NEAR, Z_FAR, heur, HDRI, osc=R.osc), o, d, 4, 50, 3, lights)
    n_nan = int(np.isnan(lit).any(axis=2).sum())
    print("lit samples with a NaN", n_nan, "of", lit.shape[0] * lit.shape[1])
    assert n_nan == LIT_NAN_SAMPLES and n_nan >= 1
    tally = _direct.new_tally()
    direct, queries = _direct.radiance_paths(R, o, d, 4, 50, 3, lights, tally=tally)
    print(tally)
    assert np.isfinite(direct).all()
    assert tally["skipped_ndl"] >= n_nan // 2 and tally["credited"] >= 10


# ---- every branch

def test_the_rooms_paths_take_every_branch():
    cam, objs, heur, names = _lit.lit_room()
    R = _direct.Reading(objs, Z_NEAR, Z_FAR, heur, HDRI)
    ocam = _oracle.OracleCamera(*scenes.camera_for_resolution(cam, 24, 16))
    lights = [names["sphere_lamp"], names["rect_lamp"], names["dark_sphere"]]
    tally = _direct.new_tally()
    values, queries = _direct.image_paths(R, ocam, 3, 50, 0x5EED, lights, tally=tally)
    unlit, unlit_q = _direct.image_paths(R, ocam, 3, 50, 0x5EED, [])
    print(tally, "queries per path", queries.mean(), "unlit", unlit_q.mean())
    assert np.isfinite(values).all()
    assert tally["skipped_ndl"] >= 10          # a shadow sample skipped for ndl_s <= 0
    assert tally["credited"] >= 100            # a shadow sample credited
    assert tally["blocked"] >= 10              # a shadow sample blocked
    assert tally["listed_met_weighted"] >= 1   # a listed object met with w < 1
    assert tally["listed_met"] > tally["listed_met_weighted"]   # ... and with w = 1: by the first ray, or after a specular bounce
    assert tally["plastic_diffuse"] >= 1 and tally["plastic_specular"] >= 1
    assert tally["taken"] == tally["credited"] + tally["blocked"]
    assert (queries <= 2 * 50 + 1).all() and queries.sum() > unlit_q.sum()
