"""The radiance queries with the sky among the lights (include/rayrs_hip.h SKY SAMPLING) on the GPU, bit for bit and count for
count against the plain-Python reading of the operation (tests/_sky.py), on both walks, in the three forms.  Every answer of the
reading on these scenes is finite, so the comparison is of bits throughout.

The scenes: the small lit room (tests/_lit.py lit_room, the local-pool route's size) with K = 0, 2 and 8 lamps beside the sky --
the eight with duplicates and a dark portal; the level-1 mesh scene with its lamp, which streams, has a hot group and a fast walk
of its own; the nine-materials row under a sphere lamp and under the sky alone.  The maps: make_hdri(32, 16), bright everywhere,
and the 9 x 5 studio map, black but for two rectangles, with an empty row of cells and texels at the clip value."""
import functools
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import _oracle
import _lit
import _sky
import rayrs_amd
from rayrs_amd import SKY, procedural, scenes
from rayrs_amd.api import Emission, Material, Object
from test_gpu_radiance import primary_rays
from test_lit import nine_materials

pytestmark = pytest.mark.gpu

MAPS = {"gradient": procedural.make_hdri(32, 16), "studio": procedural.make_studio_hdri(9, 5)}
Z_NEAR, Z_FAR = 1e-6, 1e6
# A ray aimed at a lamp's own point meets that lamp or something in front of it, never nothing: it can miss only through the z
# window.  The room once more with z_far = 6.5, for the point form (its rays are unit vectors, t is a distance): a shadow ray from
# the floor's far corners to the rectangle lamp is longer than that, misses, and is credited the background.
NEAR_Z_FAR = 6.5
S = 5
SEED = 0x5EED
W, H = 16, 12   # 192 rays, 192 points: three waves


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def floor_points(half):
    return np.array([(xi, 0.0, zi) for zi in np.linspace(-half, half, H) for xi in np.linspace(-half, half, W)])


@functools.lru_cache(maxsize=None)
def family(name, sky):
    hdri = MAPS[sky]
    z_far = NEAR_Z_FAR if name == "room_near" else Z_FAR
    if name in ("room", "room_near"):
        cam_args, objs, heur, names = _lit.lit_room()
        lamp, rect, dark = names["sphere_lamp"], names["rect_lamp"], names["dark_sphere"]
        lists = {"none": (), "two": (lamp, rect), "eight": (lamp, rect, dark, lamp, rect, rect, dark, lamp)}
        half = 3.5
    elif name == "mesh1_light":
        cam_args, objs, heur = scenes.mesh_scene(1, Material.LambertianDiffuse((0.8, 0.8, 0.8)), area_light=True)
        lists = {"none": (), "lamp": tuple(rayrs_amd.emitters(objs))}
        half = 4.0
    else:
        cam_args, objs, heur = nine_materials()
        objs = objs + [Object.sphere(0.5, (0.0, 4.0, 1.0), Material.LambertianDiffuse((0.8, 0.8, 0.8)), Emission.new(25.0, (1.0, 0.9, 0.8)))]
        lists = {"none": (), "lamp": tuple(rayrs_amd.emitters(objs))}
        half = 9.0
    scene = rayrs_amd.Scene(objs, Z_NEAR, z_far, heur, hdri, device=0)
    o, d = primary_rays(cam_args, W, H)
    if name == "nine":   # (the row's camera sees mostly sky at this size: the first 63 rays from above and in front, at the spheres)
        rng = np.random.default_rng(9)
        centre = np.array([(2.2 * (i % 9 - 4), 1.0, 0.0) for i in range(63)])
        eo = centre + (0.0, 4.0, 5.0) + rng.normal(size=(63, 3)) * 0.3
        o, d = np.concatenate([eo, o[63:]]), np.concatenate([centre + rng.normal(size=(63, 3)) * 0.4 - eo, d[63:]])
    fast_osc = _oracle.OracleScene(objs, Z_NEAR, z_far, heur, hdri).use_product_walk(scene, fast=True)
    readings = {False: _sky.Reading(objs, Z_NEAR, z_far, heur, hdri), True: _sky.Reading(objs, Z_NEAR, z_far, heur, hdri, osc=fast_osc, traversal=2)}
    p = floor_points(half)
    nrm = np.tile((0.0, 1.0, 0.0), (len(p), 1))
    assert len(o) == len(p) == 192
    for x in (o, d, p, nrm):
        x.setflags(write=False)
    return SimpleNamespace(cam_args=scenes.camera_for_resolution(cam_args, 24, 16), o=o, d=d, p=p, nrm=nrm, scene=scene, readings=readings,
                           lists=lists, info=scene.info(), tally=_sky.new_tally())


@functools.lru_cache(maxsize=None)
def expected(name, sky, which, what, fast=False, samples=S, max_bounces=50):
    """The reading's paths of the family's rays ("radiance"), points ("irradiance") or pixels ("image"): (values, queries), made
    once.  The default walk's paths at the default sizes feed the family's tally."""
    f = family(name, sky)
    R = f.readings[fast]
    tally = f.tally if not fast and samples == S and max_bounces == 50 else None
    if what == "radiance":
        return _sky.radiance_paths(R, f.o, f.d, samples, max_bounces, SEED, f.lists[which], tally=tally)
    if what == "irradiance":
        return _sky.irradiance_paths(R, f.p, f.nrm, samples, 1e-4, max_bounces, SEED, f.lists[which], tally=tally)
    return _sky.image_paths(R, _oracle.OracleCamera(*f.cam_args), samples, max_bounces, SEED, f.lists[which], tally=tally)


def check(got, values, queries, chunk, what):
    rad, cnt = got
    want_rad, want_cnt = _sky.answers(values, queries, chunk)
    assert np.isfinite(want_rad).all(), what
    assert rad.dtype == np.float64 and cnt.dtype == np.uint32 and rad.shape == want_rad.shape and cnt.shape == want_cnt.shape, what
    bad = np.flatnonzero(cnt != want_cnt)
    assert len(bad) == 0, (what, "queries", len(bad), [(int(i), int(cnt[i]), int(want_cnt[i])) for i in bad[:5]])
    bad = np.flatnonzero((bits(rad) != bits(want_rad)).any(axis=1))
    assert len(bad) == 0, (what, "radiance", len(bad), [(int(i), rad[i].tolist(), want_rad[i].tolist()) for i in bad[:3]])


def with_sky(lamps):
    return list(lamps) + [SKY]


CASES = [("room", "studio", "two"), ("room", "gradient", "none"), ("room", "studio", "eight"), ("mesh1_light", "gradient", "lamp"),
         ("mesh1_light", "studio", "none"), ("nine", "studio", "lamp"), ("nine", "gradient", "none")]


# ------------------------------------------------------------------------------------------------------ parity

@pytest.mark.parametrize("name,sky,which", CASES)
def test_sky_radiance_and_queries_are_the_readings(name, sky, which):
    f = family(name, sky)
    assert (f.info["local_pool"] == 1) == (name != "mesh1_light"), f.info
    lights = with_sky(f.lists[which])
    for fast in (False, True):
        values, queries = expected(name, sky, which, "radiance", fast)
        check(f.scene.radiance(f.o, f.d, samples=S, seed=SEED, sample_chunk=2, fast_traversal=fast, queries=True, lights=lights, direct=True),
              values, queries, 2, (name, sky, which, fast))
    direct = f.scene.radiance(f.o, f.d, samples=S, seed=SEED, lights=list(f.lists[which]), direct=True)
    got = f.scene.radiance(f.o, f.d, samples=S, seed=SEED, lights=lights, direct=True)
    # (the sky in the list changes the answers of the rays that meet a diffuse surface: few of the nine-materials row's do)
    assert (bits(direct) != bits(got)).any(axis=1).sum() >= 10
    assert np.isfinite(got).all()


@pytest.mark.parametrize("name,sky,which", CASES + [("room_near", "studio", "two")])
def test_sky_irradiance_at_points_is_the_readings(name, sky, which):
    f = family(name, sky)
    lights = with_sky(f.lists[which])
    for fast in (False, True):
        values, queries = expected(name, sky, which, "irradiance", fast)
        check(f.scene.irradiance(f.p, f.nrm, samples=S, bias=1e-4, seed=SEED, sample_chunk=2, fast_traversal=fast, queries=True, lights=lights,
                                 direct=True), values, queries, 2, (name, sky, which, fast))


@pytest.mark.parametrize("name,sky,which", [("room", "studio", "eight"), ("mesh1_light", "gradient", "lamp"), ("nine", "studio", "none")])
def test_render_sky_is_the_readings(name, sky, which):
    """Both values of fast_traversal.  The image form takes the walk a render with its settings takes: the fast walk on the mesh
    scene, which streams; on the local-pool-sized scenes a frame takes the default walk whatever is asked."""
    f = family(name, sky)
    cam = rayrs_amd.Camera(*f.cam_args)
    assert (cam.x_pixels(), cam.y_pixels()) == (24, 16)
    for fast in (False, True):
        values, queries = expected(name, sky, which, "image", fast and f.info["local_pool"] == 0, samples=3)
        img, cnt = rayrs_amd.render_lit(f.scene, cam, 3, with_sky(f.lists[which]), seed=SEED, sample_chunk=2, fast_traversal=fast, queries=True,
                                        direct=True)
        assert img.shape == (16, 24, 3) and cnt.shape == (16, 24)
        check((img.reshape(-1, 3), cnt.reshape(-1)), values, queries, 2, (name, sky, which, "image", fast))


@pytest.mark.parametrize("max_bounces", [0, 1])
def test_one_sample_and_the_bounce_bound(max_bounces):
    """S = 1 at max_bounces 50 (with the max_bounces = 1 case), and the bound itself: 0 is +0 and no query, no shadow query
    either; with 1 the shadow sample of the one bounce is traced and credited."""
    f = family("room", "studio")
    lights = with_sky(f.lists["two"])
    if max_bounces == 0:
        for call, a, b, kw in ((f.scene.radiance, f.o, f.d, {}), (f.scene.irradiance, f.p, f.nrm, dict(bias=1e-4))):
            rad, cnt = call(a, b, samples=3, max_bounces=0, queries=True, lights=lights, direct=True, **kw)
            assert rad.shape == (len(a), 3) and not bits(rad).any() and not cnt.any()
        return
    for what, call, a, b, kw in (("radiance", f.scene.radiance, f.o, f.d, {}), ("irradiance", f.scene.irradiance, f.p, f.nrm, dict(bias=1e-4))):
        values, queries = expected("room", "studio", "two", what, samples=1)
        check(call(a, b, samples=1, seed=SEED, queries=True, lights=lights, direct=True, **kw), values, queries, 0, (what, "S = 1"))
        values, queries = expected("room", "studio", "two", what, max_bounces=1)
        check(call(a, b, samples=S, seed=SEED, max_bounces=1, sample_chunk=2, queries=True, lights=lights, direct=True, **kw), values, queries, 2,
              (what, "one bounce"))
        assert queries.max() == (2 if what == "radiance" else 3)


def test_the_comparisons_are_not_vacuous():
    """From the reading alone, over the default walk's paths of the tests above: the sky is drawn, credited, blocked and skipped, a
    ray aimed at it meets a lamp, a ray aimed at a lamp is credited the background, and a path's own ray escapes with w < 1."""
    for name, sky, which in CASES:
        expected(name, sky, which, "radiance"), expected(name, sky, which, "irradiance")
    for name, sky in (("room", "studio"), ("mesh1_light", "gradient"), ("nine", "studio")):
        t = family(name, sky).tally
        print(name, sky, t)
        assert t["sky_credited"] >= 100 and t["sky_blocked"] >= 10 and t["sky_skipped_ndl"] >= 10, (name, t)
        assert t["miss_weighted"] >= 100 and t["miss_unweighted"] >= 10, (name, t)
    room, nine = family("room", "studio").tally, family("nine", "studio").tally
    assert room["sky_met_lamp"] >= 1 and room["lamp_credited"] >= 100
    expected("room_near", "studio", "two", "irradiance")
    near = family("room_near", "studio").tally
    print("room_near", near)
    assert near["lamp_missed"] >= 10 and near["lamp_credited"] >= 100
    assert room["plastic_diffuse"] >= 1 and room["plastic_specular"] >= 1 and nine["plastic_diffuse"] >= 1 and nine["plastic_specular"] >= 1


# ------------------------------------------------------------------------------------------------------ the interface

def test_repeats_of_sky_are_one_sky_and_its_place_in_the_list_does_not_matter():
    f = family("room", "studio")
    lamps = list(f.lists["two"])
    kw = dict(samples=S, seed=SEED, sample_chunk=2, queries=True, direct=True)
    a = f.scene.radiance(f.o, f.d, lights=lamps + [SKY], **kw)
    b = f.scene.radiance(f.o, f.d, lights=[SKY, lamps[0], SKY, lamps[1]], **kw)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])


def test_a_slice_with_its_index_base_is_the_slice_of_the_whole():
    f = family("mesh1_light", "gradient")
    kw = dict(samples=S, seed=SEED, sample_chunk=2, queries=True, lights=with_sky(f.lists["lamp"]), direct=True)
    rad, cnt = f.scene.radiance(f.o, f.d, **kw)
    n = len(f.o)
    for a, b in ((0, 1), (1, 70), (70, 191), (191, n)):
        r, c = f.scene.radiance(f.o[a:b], f.d[a:b], index_base=a, **kw)
        assert np.array_equal(c, cnt[a:b]) and np.array_equal(bits(r), bits(rad[a:b])), (a, b)
    irr, icnt = f.scene.irradiance(f.p, f.nrm, bias=1e-4, **kw)
    r, c = f.scene.irradiance(f.p[7:140], f.nrm[7:140], bias=1e-4, index_base=7, **kw)
    assert np.array_equal(c, icnt[7:140]) and np.array_equal(bits(r), bits(irr[7:140]))
    for call in (f.scene.radiance, f.scene.irradiance):
        r0, c0 = call(np.zeros((0, 3)), np.zeros((0, 3)), samples=3, queries=True, lights=[SKY], direct=True)
        assert r0.shape == (0, 3) and c0.shape == (0,)


def test_device_tensors_on_a_stream_give_the_host_paths_bits():
    """tests/_sky_torch_child.py, in a process of its own (torch has to be imported before the library is loaded)."""
    pytest.importorskip("torch")
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_sky_torch_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "device path ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_a_render_and_a_direct_call_are_the_same_before_and_after_a_batch_of_sky_calls():
    f = family("mesh1_light", "studio")
    cam = rayrs_amd.Camera(*f.cam_args)
    lamps = list(family("mesh1_light", "gradient").lists["lamp"])
    before, st0 = rayrs_amd.render(f.scene, cam, 4, out_f64=True)
    direct0 = f.scene.radiance(f.o, f.d, samples=S, lights=lamps, direct=True)
    for fast in (False, True):
        f.scene.radiance(f.o, f.d, samples=S, sample_chunk=2, fast_traversal=fast, lights=lamps + [SKY], direct=True)
        f.scene.irradiance(f.p, f.nrm, samples=8, bias=1e-4, fast_traversal=fast, lights=[SKY], direct=True)
        rayrs_amd.render_lit(f.scene, cam, 2, [SKY], fast_traversal=fast, direct=True)
    after, st1 = rayrs_amd.render(f.scene, cam, 4, out_f64=True)
    direct1 = f.scene.radiance(f.o, f.d, samples=S, lights=lamps, direct=True)
    assert before.tobytes() == after.tobytes() and direct0.tobytes() == direct1.tobytes()
    assert st0["rays"] == st1["rays"] and st0["paths"] == st1["paths"]
