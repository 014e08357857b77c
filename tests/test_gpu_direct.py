"""The radiance queries with direct lighting (include/rayrs_hip.h DIRECT LIGHTING) on the GPU, bit for bit and count for count
against the plain-Python reading of the operation (tests/_direct.py), on both walks, in the three forms.  Every answer of the
reading on these scenes is finite, so the comparison is of bits throughout.

The scenes: the small lit room (tests/_lit.py lit_room, the local-pool route's size) with K = 1 and with K = 8 -- duplicates and a
dark portal; the lamp box (rectangles on all six axes and two spheres, K = 8); the level-1 mesh scene, which streams and whose
listed lamp is a Lambertian rectangle that paths scatter on (LIGHT SAMPLING makes NaN there); the nine-materials row under a
sphere lamp."""
import functools
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import _direct
import _lit
import _oracle
import rayrs_amd
from rayrs_amd import procedural, scenes
from rayrs_amd.api import Emission, Material, Object
from test_gpu_radiance import primary_rays
from test_lit import nine_materials

pytestmark = pytest.mark.gpu

HDRI = procedural.make_hdri(128, 64)
Z_NEAR, Z_FAR = 1e-6, 1e6
S = 5
SEED = 0x5EED
W, H = 16, 12   # 192 rays: three waves


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def make_family(cam_args, objs, heur, lists, points, extra_rays=None):
    scene = rayrs_amd.Scene(objs, Z_NEAR, Z_FAR, heur, HDRI, device=0)
    o, d = primary_rays(cam_args, W, H)
    if extra_rays is not None:
        o, d = np.concatenate([extra_rays[0], o]), np.concatenate([extra_rays[1], d])
    fast_osc = _oracle.OracleScene(objs, Z_NEAR, Z_FAR, heur, HDRI).use_product_walk(scene, fast=True)
    readings = {False: _direct.Reading(objs, Z_NEAR, Z_FAR, heur, HDRI),
                True: _direct.Reading(objs, Z_NEAR, Z_FAR, heur, HDRI, osc=fast_osc, traversal=2)}
    nrm = np.tile((0.0, 1.0, 0.0), (len(points), 1))
    for x in (o, d, points, nrm):
        x.setflags(write=False)
    return SimpleNamespace(objs=objs, heur=heur, cam_args=scenes.camera_for_resolution(cam_args, 24, 16), o=o, d=d, scene=scene,
                           readings=readings, lists=lists, p=points, nrm=nrm, info=scene.info(), tally=_direct.new_tally())


def floor_points(half, n=7):
    x = np.linspace(-half, half, n)
    return np.array([(xi, 0.0, zi) for zi in x for xi in x])


@functools.lru_cache(maxsize=None)
def family(name):
    if name == "room":
        cam_args, objs, heur, names = _lit.lit_room()
        lamp, rect, dark = names["sphere_lamp"], names["rect_lamp"], names["dark_sphere"]
        points = np.concatenate([floor_points(3.5), [(0.0, 2.5, 0.0), (0.05, 2.45, -0.1)]])   # the last two: inside the sphere lamp
        return make_family(cam_args, objs, heur, {"one": (lamp,), "eight": (lamp, rect, dark, lamp, rect, rect, dark, lamp), "portal": (dark,)}, points)
    if name == "lamp_box":
        cam_args, objs, heur, names = _lit.lamp_box()
        assert len(names["lights"]) == 8
        return make_family(cam_args, objs, heur, {"all": names["lights"], "one": (names["rect"]["ZRev"],)}, floor_points(3.5))
    if name == "mesh1_light":
        cam_args, objs, heur = scenes.mesh_scene(1, Material.LambertianDiffuse((0.8, 0.8, 0.8)), area_light=True)
        return make_family(cam_args, objs, heur, {"emitters": tuple(rayrs_amd.emitters(objs))}, floor_points(4.0), extra_rays=_direct.lamp_rays())
    cam_args, objs, heur = nine_materials()
    objs = objs + [Object.sphere(0.5, (0.0, 4.0, 1.0), Material.LambertianDiffuse((0.8, 0.8, 0.8)), Emission.new(25.0, (1.0, 0.9, 0.8)))]
    lights = tuple(rayrs_amd.emitters(objs))
    assert len(lights) == 1
    # (the row's camera sees mostly sky at this size: 63 more rays from above and in front, aimed at the nine spheres)
    rng = np.random.default_rng(9)
    centre = np.array([(2.2 * (i % 9 - 4), 1.0, 0.0) for i in range(63)])
    o = centre + (0.0, 4.0, 5.0) + rng.normal(size=(63, 3)) * 0.3
    return make_family(cam_args, objs, heur, {"lamp": lights}, floor_points(9.0), extra_rays=(o, centre + rng.normal(size=(63, 3)) * 0.4 - o))


def expected(name, which, what, fast=False, samples=S, first=0, n=None, max_bounces=50):
    """The reading's paths of the family's rays (what = "radiance"), points ("irradiance") or pixels ("image"): (values, queries),
    made once.  The default walk's paths at the default sizes feed the family's tally."""
    return _expected(name, which, what, fast, samples, first, n, max_bounces)


@functools.lru_cache(maxsize=None)
def _expected(name, which, what, fast, samples, first, n, max_bounces):
    f = family(name)
    R = f.readings[fast]
    lights = f.lists[which] if which else ()
    tally = f.tally if not fast and samples == S and n is None and max_bounces == 50 and lights else None
    if what == "radiance":
        last = None if n is None else first + n
        return _direct.radiance_paths(R, f.o[first:last], f.d[first:last], samples, max_bounces, SEED, lights, index_base=first, tally=tally)
    if what == "irradiance":
        return _direct.irradiance_paths(R, f.p, f.nrm, samples, 1e-4, max_bounces, SEED, lights, tally=tally)
    return _direct.image_paths(R, _oracle.OracleCamera(*f.cam_args), samples, max_bounces, SEED, lights, tally=tally)


def check(got, values, queries, chunk, what):
    rad, cnt = got
    want_rad, want_cnt = _direct.answers(values, queries, chunk)
    assert np.isfinite(want_rad).all(), what
    assert rad.dtype == np.float64 and cnt.dtype == np.uint32 and rad.shape == want_rad.shape and cnt.shape == want_cnt.shape, what
    bad = np.flatnonzero(cnt != want_cnt)
    assert len(bad) == 0, (what, "queries", len(bad), [(int(i), int(cnt[i]), int(want_cnt[i])) for i in bad[:5]])
    bad = np.flatnonzero((bits(rad) != bits(want_rad)).any(axis=1))
    assert len(bad) == 0, (what, "radiance", len(bad), [(int(i), rad[i].tolist(), want_rad[i].tolist()) for i in bad[:3]])


CASES = [("room", "one"), ("room", "eight"), ("room", "portal"), ("lamp_box", "all"), ("lamp_box", "one"), ("mesh1_light", "emitters"),
         ("nine", "lamp")]
CHUNKS = (0, 1, 2, S + 2)   # one chunk; a chunk per sample; a chunk that does not divide S; a chunk above S


# ------------------------------------------------------------------------------------------------------ parity

@pytest.mark.parametrize("name,which", CASES)
def test_direct_radiance_and_queries_are_the_readings(name, which):
    f = family(name)
    assert (f.info["local_pool"] == 1) == (name != "mesh1_light"), f.info
    for fast in (False, True):
        values, queries = expected(name, which, "radiance", fast)
        for chunk in CHUNKS:
            check(f.scene.radiance(f.o, f.d, samples=S, seed=SEED, sample_chunk=chunk, fast_traversal=fast, queries=True, lights=f.lists[which],
                                   direct=True), values, queries, chunk, (name, which, fast, chunk))
    unlit = f.scene.radiance(f.o, f.d, samples=S, seed=SEED)
    lit = f.scene.radiance(f.o, f.d, samples=S, seed=SEED, lights=f.lists[which])
    direct = f.scene.radiance(f.o, f.d, samples=S, seed=SEED, lights=f.lists[which], direct=True)
    if which != "portal":   # (the strategy changes the answers; a dark portal alone changes the draws, and so the paths)
        assert (bits(unlit) != bits(direct)).any(axis=1).sum() >= 20
    assert (bits(lit) != bits(direct)).any(axis=1).sum() >= 20
    assert np.isfinite(direct).all()


@pytest.mark.parametrize("name,which", CASES)
def test_direct_irradiance_at_points_is_the_readings(name, which):
    f = family(name)
    for fast in (False, True):
        values, queries = expected(name, which, "irradiance", fast)
        for chunk in (0, 2):
            check(f.scene.irradiance(f.p, f.nrm, samples=S, bias=1e-4, seed=SEED, sample_chunk=chunk, fast_traversal=fast, queries=True,
                                     lights=f.lists[which], direct=True), values, queries, chunk, (name, which, fast, chunk))


@pytest.mark.parametrize("name,which", [("room", "eight"), ("lamp_box", "all"), ("mesh1_light", "emitters"), ("nine", "lamp")])
def test_render_direct_is_the_readings(name, which):
    """Both values of fast_traversal.  The image form takes the walk a render with its settings takes: the fast walk on the
    mesh scene, which streams; on the three local-pool-sized scenes a frame takes the default walk whatever is asked."""
    f = family(name)
    cam = rayrs_amd.Camera(*f.cam_args)
    assert (cam.x_pixels(), cam.y_pixels()) == (24, 16)
    for fast in (False, True):
        values, queries = expected(name, which, "image", fast and f.info["local_pool"] == 0, samples=3)
        for chunk in (0, 2):
            img, cnt = rayrs_amd.render_lit(f.scene, cam, 3, f.lists[which], seed=SEED, sample_chunk=chunk, fast_traversal=fast, queries=True,
                                            direct=True)
            assert img.shape == (16, 24, 3) and cnt.shape == (16, 24)
            check((img.reshape(-1, 3), cnt.reshape(-1)), values, queries, chunk, (name, which, "image", fast, chunk))


def test_the_comparisons_are_not_vacuous():
    """From the reading alone, over the default walk's paths of the tests above: every branch of the turn is taken."""
    for name, which in CASES:
        expected(name, which, "radiance"), expected(name, which, "irradiance")
    room, box, mesh, nine = (family(n).tally for n in ("room", "lamp_box", "mesh1_light", "nine"))
    print("room", room, "lamp_box", box, "mesh1_light", mesh, "nine", nine)
    for t in (room, box, mesh, nine):
        assert t["credited"] >= 100 and t["skipped_ndl"] >= 1 and t["taken"] == t["credited"] + t["blocked"]
    assert room["blocked"] >= 10 and box["blocked"] >= 10 and nine["blocked"] >= 10
    assert room["listed_met_weighted"] >= 1 and room["listed_met"] > room["listed_met_weighted"]
    assert mesh["listed_met_weighted"] >= 1 and mesh["skipped_ndl"] >= 100   # (the lamp drawing itself)
    assert room["plastic_diffuse"] >= 1 and room["plastic_specular"] >= 1 and nine["plastic_diffuse"] >= 1 and nine["plastic_specular"] >= 1
    c, r = np.array((0.0, 2.5, 0.0)), 0.25
    p = family("room").p
    assert ((((p + family("room").nrm * 1e-4) - c) ** 2).sum(axis=1) < r * r).sum() >= 1   # a point inside a sphere of the list


# ------------------------------------------------------------------------------------------------------ no lights

@pytest.mark.parametrize("name", ["mesh1_light", "room"])
def test_an_empty_list_is_the_unlit_query_and_the_unlit_render(name):
    f = family(name)
    cam = rayrs_amd.Camera(*f.cam_args)
    for fast in (False, True):
        for chunk in (0, 2):
            kw = dict(samples=S, seed=SEED, sample_chunk=chunk, fast_traversal=fast, queries=True)
            a, b = f.scene.radiance(f.o, f.d, **kw), f.scene.radiance(f.o, f.d, lights=[], direct=True, **kw)
            assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]), (name, fast, chunk)
            a, b = f.scene.irradiance(f.p, f.nrm, bias=1e-4, **kw), f.scene.irradiance(f.p, f.nrm, bias=1e-4, lights=[], direct=True, **kw)
            assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]), (name, fast, chunk)
            img, st = rayrs_amd.render(f.scene, cam, S, seed=SEED, sample_chunk=chunk, out_f64=True, fast_traversal=fast)
            got, cnt = rayrs_amd.render_lit(f.scene, cam, S, [], seed=SEED, sample_chunk=chunk, fast_traversal=fast, queries=True, direct=True)
            assert img.tobytes() == got.tobytes() and int(cnt.sum()) == st["rays"], (name, fast, chunk)
    assert (img != 0.0).any(axis=2).sum() >= 300


# ------------------------------------------------------------------------------------------------------ the bounce bound

@pytest.mark.parametrize("max_bounces", [0, 1, 2])
def test_the_bounce_bound_does_not_count_the_shadow_query(max_bounces):
    """max_bounces = 0: +0 and no query, no shadow query either.  1 and 2: the reading's; the shadow sample at the last allowed
    bounce is traced and credited -- with one bounce a ray that meets the dark floor first has two queries and a value."""
    f = family("room")
    lights = f.lists["eight"]
    if max_bounces == 0:
        for call, a, b, kw in ((f.scene.radiance, f.o, f.d, {}), (f.scene.irradiance, f.p, f.nrm, dict(bias=1e-4))):
            rad, cnt = call(a, b, samples=3, max_bounces=0, queries=True, lights=lights, direct=True, **kw)
            assert rad.shape == (len(a), 3) and not bits(rad).any() and not cnt.any()
        return
    values, queries = expected("room", "eight", "radiance", max_bounces=max_bounces)
    check(f.scene.radiance(f.o, f.d, samples=S, seed=SEED, max_bounces=max_bounces, queries=True, lights=lights, direct=True), values, queries, 0,
          ("radiance", max_bounces))
    assert queries.max() == 2 * max_bounces
    if max_bounces == 1:
        first = np.array([f.readings[False].osc.intersect(o, d, Z_NEAR, Z_FAR)[0] for o, d in zip(f.o, f.d)])
        floor = first == 0
        credited = floor[:, None] & (queries == 2) & (values != 0.0).any(axis=2)
        print("floor rays", int(floor.sum()), "samples with a credited last-bounce shadow sample", int(credited.sum()))
        assert credited.sum() >= 50
    values, queries = expected("room", "eight", "irradiance", max_bounces=max_bounces)
    check(f.scene.irradiance(f.p, f.nrm, samples=S, bias=1e-4, seed=SEED, max_bounces=max_bounces, queries=True, lights=lights, direct=True),
          values, queries, 0, ("irradiance", max_bounces))
    assert queries.max() == 2 * max_bounces + 1


# ------------------------------------------------------------------------------------------------------ the schedule

@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_batches_around_a_wave(n):
    f = family("room")
    a = 100   # (rays that meet the room's objects)
    values, queries = expected("room", "eight", "radiance", first=a, n=n)
    got = f.scene.radiance(f.o[a:a + n], f.d[a:a + n], samples=S, seed=SEED, index_base=a, sample_chunk=2, queries=True, lights=f.lists["eight"],
                           direct=True)
    check(got, values, queries, 2, n)


def test_a_whole_wave_of_identical_rays():
    """64 copies of one ray that meets the floor: their keys differ (index_base + i), their first hit does not."""
    f = family("room")
    first = np.array([f.readings[False].osc.intersect(o, d, Z_NEAR, Z_FAR)[0] for o, d in zip(f.o, f.d)])
    i = int(np.flatnonzero(first == 0)[0])
    o, d = np.tile(f.o[i], (64, 1)), np.tile(f.d[i], (64, 1))
    lights = f.lists["eight"]
    for fast in (False, True):
        values, queries = _direct.radiance_paths(f.readings[fast], o, d, S, 50, SEED, lights)
        check(f.scene.radiance(o, d, samples=S, seed=SEED, fast_traversal=fast, queries=True, lights=lights, direct=True), values, queries, 0,
              ("identical", fast))
    assert len({v.tobytes() for v in values[:, 0]}) >= 32


def test_a_slice_with_its_index_base_is_the_slice_of_the_whole():
    f = family("lamp_box")
    kw = dict(samples=S, seed=SEED, sample_chunk=2, queries=True, lights=f.lists["all"], direct=True)
    rad, cnt = f.scene.radiance(f.o, f.d, **kw)
    n = len(f.o)
    for a, b in ((0, 1), (1, 70), (70, 191), (191, n)):
        r, c = f.scene.radiance(f.o[a:b], f.d[a:b], index_base=a, **kw)
        assert np.array_equal(c, cnt[a:b]) and np.array_equal(bits(r), bits(rad[a:b])), (a, b)
    irr, icnt = f.scene.irradiance(f.p, f.nrm, bias=1e-4, **kw)
    r, c = f.scene.irradiance(f.p[7:40], f.nrm[7:40], bias=1e-4, index_base=7, **kw)
    assert np.array_equal(c, icnt[7:40]) and np.array_equal(bits(r), bits(irr[7:40]))
    for call in (f.scene.radiance, f.scene.irradiance):
        r0, c0 = call(np.zeros((0, 3)), np.zeros((0, 3)), samples=3, queries=True, lights=f.lists["all"], direct=True)
        assert r0.shape == (0, 3) and c0.shape == (0,)


@pytest.mark.parametrize("knobs", [(1, 1, 1), (64, 64, 64), (32, 16, 8)], ids=["1-1-1", "64-64-64", "32-16-8"])
def test_the_thresholds_give_the_same_bits(knobs):
    """The lit kernels' private hook (Scene.lab_radiance_tuning) sets the direct kernels' thresholds too: every setting gives
    the reading's bits, which the default setting gives in the parity tests above."""
    for name, which in (("mesh1_light", "emitters"), ("room", "eight")):
        f = family(name)
        try:
            f.scene.lab_radiance_tuning(*knobs)
            for fast in (False, True):
                values, queries = expected(name, which, "radiance", fast)
                check(f.scene.radiance(f.o, f.d, samples=S, seed=SEED, sample_chunk=2, fast_traversal=fast, queries=True, lights=f.lists[which],
                                       direct=True), values, queries, 2, (name, knobs, fast))
            values, queries = expected(name, which, "irradiance")
            check(f.scene.irradiance(f.p, f.nrm, samples=S, bias=1e-4, seed=SEED, sample_chunk=2, queries=True, lights=f.lists[which], direct=True),
                  values, queries, 2, (name, knobs, "irradiance"))
        finally:
            f.scene.lab_radiance_tuning(0, 0, 0)


def test_device_tensors_on_a_stream_give_the_host_paths_bits():
    """tests/_direct_torch_child.py, in a process of its own (torch has to be imported before the library is loaded)."""
    pytest.importorskip("torch")
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_direct_torch_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "device path ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_a_render_is_the_same_before_and_after_a_batch_of_direct_calls():
    f = family("mesh1_light")
    cam = rayrs_amd.Camera(*f.cam_args)
    before, st0 = rayrs_amd.render(f.scene, cam, 4, out_f64=True)
    lights = f.lists["emitters"]
    for fast in (False, True):
        f.scene.radiance(f.o, f.d, samples=S, sample_chunk=2, fast_traversal=fast, lights=lights, direct=True)
        f.scene.irradiance(f.p, f.nrm, samples=8, bias=1e-4, fast_traversal=fast, lights=lights, direct=True)
        rayrs_amd.render_lit(f.scene, cam, 2, lights, fast_traversal=fast, direct=True)
    after, st1 = rayrs_amd.render(f.scene, cam, 4, out_f64=True)
    assert before.tobytes() == after.tobytes()
    assert st0["rays"] == st1["rays"] and st0["paths"] == st1["paths"]
