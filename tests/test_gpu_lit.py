"""The radiance queries with light sampling (include/rayrs_hip.h LIGHT SAMPLING) on the GPU, count for count and bit for bit
against the plain-Python reading of the operation (tests/_lit.py), on both walks, S = 5 with sample_chunk 0 and 2.  Where the
operation itself makes a NaN (the header: "whatever IEEE gives" -- a Lambertian rectangle of the list drawing itself, on
mesh3_light) the NaN places must coincide and every other component agree in bits, as tests/test_gpu_nonfinite_rays.py compares.

mesh3_light is the streaming route's scene with a hot group, its list emitters(objs); the small lit room (tests/_lit.py
lit_room) is of the local-pool route's size, with two lists of K = 3: lamp, rectangle and the dark sphere; lamp, rectangle and
the lamp once more."""
import functools
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import _lit
import _nonfinite_rays as N
import _oracle
import _radiance
import rayrs_amd
from _nonfinite import assert_same_frame_nan_aware
from rayrs_amd import procedural, scenes
from rayrs_amd.api import Material
from test_gpu_radiance import primary_rays

pytestmark = pytest.mark.gpu

HDRI = procedural.make_hdri(128, 64)
Z_NEAR, Z_FAR = 1e-6, 1e6
S = 5
SEED = 0x5EED


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def make_family(cam_args, objs, heur, w, h, lists, points):
    scene = rayrs_amd.Scene(objs, Z_NEAR, Z_FAR, heur, HDRI, device=0)
    o, d = primary_rays(cam_args, w, h)
    fast_osc = _oracle.OracleScene(objs, Z_NEAR, Z_FAR, heur, HDRI).use_product_walk(scene, fast=True)
    readings = {False: _lit.Reading(objs, Z_NEAR, Z_FAR, heur, HDRI),
                True: _lit.Reading(objs, Z_NEAR, Z_FAR, heur, HDRI, osc=fast_osc, traversal=2)}
    nrm = np.tile((0.0, 1.0, 0.0), (len(points), 1))
    points.setflags(write=False), nrm.setflags(write=False)
    return SimpleNamespace(objs=objs, heur=heur, cam_args=scenes.camera_for_resolution(cam_args, w, h), w=w, h=h, o=o, d=d, scene=scene,
                           readings=readings, lists=lists, p=points, nrm=nrm, info=scene.info(), tally=_lit.new_tally())


@functools.lru_cache(maxsize=None)
def family(name):
    if name == "mesh3_light":
        cam_args, objs, heur = scenes.mesh_scene(3, Material.LambertianDiffuse((0.8, 0.8, 0.8)), area_light=True)
        x = np.linspace(-4.0, 4.0, 8)
        points = np.array([(xi, 0.0, zi) for zi in x for xi in x])
        return make_family(cam_args, objs, heur, 32, 24, {"emitters": tuple(rayrs_amd.emitters(objs))}, points)
    cam_args, objs, heur, names = _lit.lit_room()
    x = np.linspace(-3.5, 3.5, 8)
    points = np.array([(xi, 0.0, zi) for zi in x for xi in x] + [(0.0, 2.5, 0.0), (0.05, 2.45, -0.1)])   # the last two: inside the sphere lamp
    lists = {"dark": (names["sphere_lamp"], names["rect_lamp"], names["dark_sphere"]),
             "duplicate": (names["sphere_lamp"], names["rect_lamp"], names["sphere_lamp"])}
    f = make_family(cam_args, objs, heur, 32, 24, lists, points)
    f.names = names
    return f


@functools.lru_cache(maxsize=None)
def expected(name, which, what, fast=False, samples=S, first=0, n=None, max_bounces=50):
    """The reading's paths of the family's rays (what = "radiance"), points ("irradiance") or pixels ("image"): (values, queries).
    The default walk's paths at the default sizes feed the family's tally."""
    f = family(name)
    R = f.readings[fast]
    lights = f.lists[which] if which else ()
    tally = f.tally if not fast and samples == S and n is None and lights else None
    if what == "radiance":
        last = None if n is None else first + n
        return _lit.radiance_paths(R, f.o[first:last], f.d[first:last], samples, max_bounces, SEED, lights, index_base=first, tally=tally)
    if what == "irradiance":
        return _lit.irradiance_paths(R, f.p, f.nrm, samples, 1e-4, max_bounces, SEED, lights, tally=tally)
    return _lit.image_paths(R, _oracle.OracleCamera(*f.cam_args), samples, max_bounces, SEED, lights, tally=tally)


def check(got, values, queries, chunk, what):
    rad, cnt = got
    want_rad, want_cnt = _radiance.answers(values, queries, chunk)
    assert rad.dtype == np.float64 and cnt.dtype == np.uint32 and rad.shape == want_rad.shape and cnt.shape == want_cnt.shape, what
    bad = np.flatnonzero(cnt != want_cnt)
    assert len(bad) == 0, (what, "queries", len(bad), [(int(i), int(cnt[i]), int(want_cnt[i])) for i in bad[:5]])
    assert_same_frame_nan_aware(rad, want_rad, str(what))


CASES = [("mesh3_light", "emitters"), ("room", "dark"), ("room", "duplicate")]


# ------------------------------------------------------------------------------------------------------ parity

@pytest.mark.parametrize("name,which", CASES)
def test_lit_radiance_and_queries_are_the_readings(name, which):
    f = family(name)
    assert (f.info["local_pool"] == 1) == (name == "room") and (f.info["hot_count"] >= 1) == (name == "mesh3_light")
    for fast in (False, True):
        values, queries = expected(name, which, "radiance", fast)
        for chunk in (0, 2):
            check(f.scene.radiance(f.o, f.d, samples=S, seed=SEED, sample_chunk=chunk, fast_traversal=fast, queries=True, lights=f.lists[which]),
                  values, queries, chunk, (name, which, fast, chunk))
    unlit = f.scene.radiance(f.o, f.d, samples=S, seed=SEED)
    lit = f.scene.radiance(f.o, f.d, samples=S, seed=SEED, lights=f.lists[which])
    assert (bits(unlit) != bits(lit)).any(axis=1).sum() >= 100   # (the lights change the answers)


@pytest.mark.parametrize("name,which", CASES)
def test_lit_irradiance_at_points_is_the_readings(name, which):
    f = family(name)
    for fast in (False, True):
        values, queries = expected(name, which, "irradiance", fast)
        for chunk in (0, 2):
            check(f.scene.irradiance(f.p, f.nrm, samples=S, bias=1e-4, seed=SEED, sample_chunk=chunk, fast_traversal=fast, queries=True,
                                     lights=f.lists[which]), values, queries, chunk, (name, which, fast, chunk))


@pytest.mark.parametrize("name,which", [("mesh3_light", "emitters"), ("room", "dark")])
def test_render_lit_is_the_readings(name, which):
    f = family(name)
    cam = rayrs_amd.Camera(*f.cam_args)
    assert (cam.x_pixels(), cam.y_pixels()) == (32, 24)
    values, queries = expected(name, which, "image")
    for chunk in (0, 2):
        img, cnt = rayrs_amd.render_lit(f.scene, cam, S, f.lists[which], seed=SEED, sample_chunk=chunk, queries=True)
        assert img.shape == (24, 32, 3) and cnt.shape == (24, 32)
        check((img.reshape(-1, 3), cnt.reshape(-1)), values, queries, chunk, (name, which, "image", chunk))


def test_the_comparisons_are_not_vacuous():
    """From the reading alone, over the default walk's paths of the tests above."""
    room, mesh = family("room"), family("mesh3_light")
    for which in ("dark", "duplicate"):
        expected("room", which, "radiance"), expected("room", which, "irradiance")
    expected("room", "dark", "image")
    expected("mesh3_light", "emitters", "radiance"), expected("mesh3_light", "emitters", "irradiance")
    t, m = room.tally, mesh.tally
    print("room", t, "mesh3_light", m)
    assert t["light_arm"] >= 100 and t["cosine_arm"] >= 100 and m["light_arm"] >= 100 and m["cosine_arm"] >= 100
    assert t["ndl_negative"] >= 10
    assert min(t["sampled"].values()) >= 10 and min(t["hit"].values()) >= 10   # spheres and rectangles: sampled, and then hit
    assert m["blocked_by_mesh"] >= 1
    assert t["plastic_diffuse"] >= 1 and t["plastic_specular"] >= 1
    c, r = np.array((0.0, 2.5, 0.0)), 0.25
    inside = (((room.p + room.nrm * 1e-4 - c) ** 2).sum(axis=1) < r * r).sum()
    assert inside >= 1
    # a NaN of the operation's own is met (and compared) on mesh3_light, none in the room
    v, q = expected("mesh3_light", "emitters", "radiance")
    print("mesh3_light NaN paths", int(np.isnan(v).any(axis=2).sum()))
    for which in ("dark", "duplicate"):
        assert np.isfinite(expected("room", which, "radiance")[0]).all()


# ------------------------------------------------------------------------------------------------------ no lights

@pytest.mark.parametrize("name", ["mesh3_light", "room"])
def test_an_empty_list_is_the_unlit_query_and_the_unlit_render(name):
    f = family(name)
    cam = rayrs_amd.Camera(*scenes.camera_for_resolution(f.cam_args, 48, 32))
    for fast in (False, True):
        for chunk in (0, 2):
            kw = dict(samples=S, seed=SEED, sample_chunk=chunk, fast_traversal=fast, queries=True)
            a, b = f.scene.radiance(f.o, f.d, **kw), f.scene.radiance(f.o, f.d, lights=[], **kw)
            assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]), (name, fast, chunk)
            a, b = f.scene.irradiance(f.p, f.nrm, bias=1e-4, **kw), f.scene.irradiance(f.p, f.nrm, bias=1e-4, lights=[], **kw)
            assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]), (name, fast, chunk)
            img, st = rayrs_amd.render(f.scene, cam, S, seed=SEED, sample_chunk=chunk, out_f64=True, fast_traversal=fast)
            lit, cnt = rayrs_amd.render_lit(f.scene, cam, S, [], seed=SEED, sample_chunk=chunk, fast_traversal=fast, queries=True)
            assert img.tobytes() == lit.tobytes() and int(cnt.sum()) == st["rays"], (name, fast, chunk)
    assert (img != 0.0).any(axis=2).sum() >= 1000


# ------------------------------------------------------------------------------------------------------ the schedule

@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_batches_around_a_wave(n):
    f = family("room")
    a = 300   # (rays that meet the room's objects)
    values, queries = expected("room", "dark", "radiance", first=a, n=n)
    got = f.scene.radiance(f.o[a:a + n], f.d[a:a + n], samples=S, seed=SEED, index_base=a, sample_chunk=2, queries=True, lights=f.lists["dark"])
    check(got, values, queries, 2, n)


def test_a_slice_with_its_index_base_is_the_slice_of_the_whole():
    f = family("room")
    kw = dict(samples=S, seed=SEED, sample_chunk=2, queries=True, lights=f.lists["duplicate"])
    rad, cnt = f.scene.radiance(f.o, f.d, **kw)
    n = len(f.o)
    for a, b in ((0, 1), (1, 130), (130, 401), (401, n)):
        r, c = f.scene.radiance(f.o[a:b], f.d[a:b], index_base=a, **kw)
        assert np.array_equal(c, cnt[a:b]) and np.array_equal(bits(r), bits(rad[a:b])), (a, b)
    irr, icnt = f.scene.irradiance(f.p, f.nrm, bias=1e-4, **kw)
    r, c = f.scene.irradiance(f.p[7:40], f.nrm[7:40], bias=1e-4, index_base=7, **kw)
    assert np.array_equal(c, icnt[7:40]) and np.array_equal(bits(r), bits(irr[7:40]))
    for call in (f.scene.radiance, f.scene.irradiance):
        r0, c0 = call(np.zeros((0, 3)), np.zeros((0, 3)), samples=3, queries=True, lights=f.lists["dark"])
        assert r0.shape == (0, 3) and c0.shape == (0,)
        r0, c0 = call(f.o[:70], f.d[:70], samples=3, max_bounces=0, queries=True, lights=f.lists["dark"])
        assert not bits(r0).any() and not c0.any() and r0.shape == (70, 3)


def test_one_batch_of_more_than_a_launch():
    """S = 1: an item a ray and 2^20 of them a launch.  The single-sphere scene with a Lambertian sphere, which is the list (a
    dark target is legal)."""
    cam_args, objs, heur = scenes.single_sphere(Material.LambertianDiffuse((0.8, 0.6, 0.4)))
    scene = rayrs_amd.Scene(objs, Z_NEAR, Z_FAR, heur, HDRI, device=0)
    o, d = primary_rays(cam_args, 32, 16)
    reps = 2049
    big_o, big_d = np.tile(o, (reps, 1)), np.tile(d, (reps, 1))
    m, n = len(big_o), len(o)
    assert 1 << 20 < m < (1 << 20) + 1000
    kw = dict(samples=1, seed=SEED, queries=True, lights=[1])
    rad, cnt = scene.radiance(big_o, big_d, **kw)
    pieces = [scene.radiance(big_o[a:b], big_d[a:b], index_base=a, **kw) for a, b in ((0, 300001), (300001, 1048577), (1048577, m))]
    assert np.array_equal(np.concatenate([c for _, c in pieces]), cnt)
    assert np.array_equal(bits(np.concatenate([r for r, _ in pieces])), bits(rad))
    R = _lit.Reading(objs, Z_NEAR, Z_FAR, heur, HDRI)
    values, queries = _lit.radiance_paths(R, o, d, 1, 50, SEED, [1])
    check((rad[:n], cnt[:n]), values, queries, 0, "the first rays")
    values, queries = _lit.radiance_paths(R, o[-64:], d[-64:], 1, 50, SEED, [1], index_base=m - 64)
    check((rad[-64:], cnt[-64:]), values, queries, 0, "the last rays")
    assert (queries >= 2).sum() >= 10


@pytest.mark.parametrize("knobs", [(1, 1, 1), (64, 64, 64), (0, 0, 0)], ids=["1-1-1", "64-64-64", "default"])
def test_the_thresholds_give_the_same_bits(knobs):
    for name, which in (("mesh3_light", "emitters"), ("room", "dark")):
        f = family(name)
        try:
            f.scene.lab_radiance_tuning(*knobs)
            for fast in (False, True):
                values, queries = expected(name, which, "radiance", fast)
                check(f.scene.radiance(f.o, f.d, samples=S, seed=SEED, sample_chunk=2, fast_traversal=fast, queries=True, lights=f.lists[which]),
                      values, queries, 2, (name, knobs, fast))
            values, queries = expected(name, which, "irradiance")
            check(f.scene.irradiance(f.p, f.nrm, samples=S, bias=1e-4, seed=SEED, sample_chunk=2, queries=True, lights=f.lists[which]),
                  values, queries, 2, (name, knobs, "irradiance"))
        finally:
            f.scene.lab_radiance_tuning(0, 0, 0)


def test_device_tensors_on_a_stream_give_the_host_paths_bits():
    """tests/_lit_torch_child.py, in a process of its own (torch has to be imported before the library is loaded)."""
    pytest.importorskip("torch")
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lit_torch_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "device path ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_a_render_is_the_same_before_and_after_a_batch_of_lit_calls():
    f = family("mesh3_light")
    cam = rayrs_amd.Camera(*scenes.camera_for_resolution(f.cam_args, 48, 32))
    before, st0 = rayrs_amd.render(f.scene, cam, 4, out_f64=True)
    lights = f.lists["emitters"]
    for fast in (False, True):
        f.scene.radiance(f.o, f.d, samples=S, sample_chunk=2, fast_traversal=fast, lights=lights)
        f.scene.irradiance(f.p, f.nrm, samples=8, bias=1e-4, fast_traversal=fast, lights=lights)
        rayrs_amd.render_lit(f.scene, cam, 2, lights, fast_traversal=fast)
    after, st1 = rayrs_amd.render(f.scene, cam, 4, out_f64=True)
    assert before.tobytes() == after.tobytes()
    assert st0["rays"] == st1["rays"] and st0["paths"] == st1["paths"]


# ------------------------------------------------------------------------------------------------------ non-finite rays

def test_non_finite_rays_through_the_lit_route_are_the_readings():
    """The ray families of tests/_nonfinite_rays.py, in runs among mesh3_light's rays, once, on the default walk."""
    f = family("mesh3_light")
    o, d, touched = N.corrupt_in_runs(f.o, f.d, f.info["root_box"], 64)
    lights = f.lists["emitters"]
    values, queries = _lit.radiance_paths(f.readings[False], o, d, S, 50, SEED, lights)
    want, _ = _radiance.answers(values, queries, 0)
    print("corrupted rays", int(touched.sum()), "NaN answers", int(np.isnan(want).any(axis=1).sum()))
    assert touched.sum() >= 100 and np.isnan(want).any(axis=1).sum() >= 20
    for chunk in (0, 2):
        check(f.scene.radiance(o, d, samples=S, seed=SEED, sample_chunk=chunk, queries=True, lights=lights), values, queries, chunk, ("non-finite", chunk))
