"""The radiance queries with a mesh-light group among the lights (include/rayrs_hip.h MESH LIGHTS) on the GPU, bit for bit and
count for count against the plain-Python reading of the operation (tests/_mesh.py), on both walks, in the three forms.  Every answer
of the reading on these scenes is finite, so the comparison is of bits throughout.

The scenes: tests/_mesh.py's room (the lit room with a listed quad, a listed quad behind it, a listed octahedron above the sphere
lamp and an unlisted emissive triangle; f64 records) with K = 0, 2 and 8 lamps, without and with the sky -- M
from 1 to 10; its small version with the one quad, which is of the local-pool route's size; and the level-1 mesh scene with its mesh emissive and every third of its triangles listed, which streams, has a hot
group and a fast walk of its own, whose search is several levels deep and whose unlisted emissive triangles sit beside listed
ones, with its rectangle lamp or without."""
import dataclasses
import functools
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import _mesh
import _oracle
import rayrs_amd
from rayrs_amd import SKY, procedural, scenes
from rayrs_amd.api import Emission, Material
from test_gpu_radiance import primary_rays

pytestmark = pytest.mark.gpu

HDRI = procedural.make_studio_hdri(9, 5)
Z_NEAR, Z_FAR = 1e-6, 1e6
S = 5
SEED = 0x5EED
W, H = 16, 12   # 192 rays, 192 points: three waves


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def floor_points(half):
    return np.array([(xi, 0.0, zi) for zi in np.linspace(-half, half, H) for xi in np.linspace(-half, half, W)])


def mesh1_objects():
    """(camera args, objects, heuristic, the listed triangles): the level-1 mesh scene, its mesh emissive, every third listed."""
    cam_args, objs, heur = scenes.mesh_scene(1, Material.LambertianDiffuse((0.8, 0.8, 0.8)), area_light=True)
    objs = list(objs)
    assert objs[1].kind == "mesh" and len(objs) == 3
    objs[1] = dataclasses.replace(objs[1], emission=Emission.new(2.0, (1.0, 0.7, 0.5)))
    tris = rayrs_amd.mesh_emitters(objs)
    assert tris == list(range(1, 1 + len(objs[1].idx)))
    return cam_args, objs, heur, tris[::3]


@functools.lru_cache(maxsize=None)
def family(name):
    if name in ("room", "small"):
        cam_args, objs, heur, names = _mesh.mesh_room(small=name == "small")
        lamp, rect, dark = names["sphere_lamp"], names["rect_lamp"], names["dark_sphere"]
        lists = {"none": (), "two": (lamp, rect), "eight": (lamp, rect, dark, lamp, rect, rect, dark, lamp)}
        tris = names["group"]
        half = 3.5
    else:
        cam_args, objs, heur, tris = mesh1_objects()
        lists = {"none": (), "lamp": tuple(rayrs_amd.emitters(objs))}
        assert len(lists["lamp"]) == 1 and len(tris) >= 20
        half = 4.0
    scene = rayrs_amd.Scene(objs, Z_NEAR, Z_FAR, heur, HDRI, device=0)
    mesh = scene.mesh_lights(tris)
    o, d = primary_rays(cam_args, W, H)
    fast_osc = _oracle.OracleScene(objs, Z_NEAR, Z_FAR, heur, HDRI).use_product_walk(scene, fast=True)
    readings = {False: _mesh.Reading(objs, Z_NEAR, Z_FAR, heur, HDRI, tris),
                True: _mesh.Reading(objs, Z_NEAR, Z_FAR, heur, HDRI, tris, osc=fast_osc, traversal=2)}
    p = floor_points(half)
    nrm = np.tile((0.0, 1.0, 0.0), (len(p), 1))
    assert len(o) == len(p) == 192
    for x in (o, d, p, nrm):
        x.setflags(write=False)
    return SimpleNamespace(cam_args=scenes.camera_for_resolution(cam_args, 24, 16), o=o, d=d, p=p, nrm=nrm, scene=scene, mesh=mesh,
                           tris=tris, readings=readings, lists=lists, info=scene.info(), tally=_mesh.new_tally())


def lights_of(f, which, sky):
    return list(f.lists[which]) + ([SKY] if sky else [])


@functools.lru_cache(maxsize=None)
def expected(name, which, sky, what, fast=False, samples=S, max_bounces=50):
    """The reading's paths of the family's rays ("radiance"), points ("irradiance") or pixels ("image"): (values, queries), made
    once.  The default walk's paths at the default sizes feed the family's tally."""
    f = family(name)
    R = f.readings[fast]
    tally = f.tally if not fast and samples == S and max_bounces == 50 else None
    lights = lights_of(f, which, sky)
    if what == "radiance":
        return _mesh.radiance_paths(R, f.o, f.d, samples, max_bounces, SEED, lights, tally=tally)
    if what == "irradiance":
        return _mesh.irradiance_paths(R, f.p, f.nrm, samples, 1e-4, max_bounces, SEED, lights, tally=tally)
    return _mesh.image_paths(R, _oracle.OracleCamera(*f.cam_args), samples, max_bounces, SEED, lights, tally=tally)


def check(got, values, queries, chunk, what):
    rad, cnt = got
    want_rad, want_cnt = _mesh.answers(values, queries, chunk)
    assert np.isfinite(want_rad).all(), what
    assert rad.dtype == np.float64 and cnt.dtype == np.uint32 and rad.shape == want_rad.shape and cnt.shape == want_cnt.shape, what
    bad = np.flatnonzero(cnt != want_cnt)
    assert len(bad) == 0, (what, "queries", len(bad), [(int(i), int(cnt[i]), int(want_cnt[i])) for i in bad[:5]])
    bad = np.flatnonzero((bits(rad) != bits(want_rad)).any(axis=1))
    assert len(bad) == 0, (what, "radiance", len(bad), [(int(i), rad[i].tolist(), want_rad[i].tolist()) for i in bad[:3]])


CASES = [("room", "none", False), ("room", "none", True), ("room", "two", False), ("room", "two", True), ("room", "eight", False),
         ("room", "eight", True), ("mesh1", "lamp", False), ("mesh1", "lamp", True), ("mesh1", "none", False), ("mesh1", "none", True), ("small", "two", True), ("small", "none", False)]


# ------------------------------------------------------------------------------------------------------ parity

@pytest.mark.parametrize("name,which,sky", CASES)
def test_mesh_radiance_and_queries_are_the_readings(name, which, sky):
    f = family(name)
    assert (f.info["local_pool"] == 1) == (name == "small") and (f.info["compact"] == 1) == (name == "mesh1"), f.info
    lights = lights_of(f, which, sky)
    for fast in (False, True):
        values, queries = expected(name, which, sky, "radiance", fast)
        check(f.scene.radiance(f.o, f.d, samples=S, seed=SEED, sample_chunk=2, fast_traversal=fast, queries=True, lights=lights, direct=True,
                               mesh=f.mesh), values, queries, 2, (name, which, sky, fast))


@pytest.mark.parametrize("name,which,sky", CASES)
def test_mesh_irradiance_at_points_is_the_readings(name, which, sky):
    f = family(name)
    lights = lights_of(f, which, sky)
    for fast in (False, True):
        values, queries = expected(name, which, sky, "irradiance", fast)
        check(f.scene.irradiance(f.p, f.nrm, samples=S, bias=1e-4, seed=SEED, sample_chunk=2, fast_traversal=fast, queries=True, lights=lights,
                                 direct=True, mesh=f.mesh), values, queries, 2, (name, which, sky, fast))


@pytest.mark.parametrize("name,which,sky", [("room", "eight", True), ("room", "two", False), ("mesh1", "lamp", True), ("mesh1", "none", False),
                                            ("small", "two", True)])
def test_render_mesh_is_the_readings(name, which, sky):
    """Both values of fast_traversal.  The image form takes the walk a render with its settings takes: the fast walk on the mesh
    scenes, which stream (the room's twenty objects are past the local-pool route's size); on the local-pool-sized small room a
    frame takes the default walk whatever is asked."""
    f = family(name)
    cam = rayrs_amd.Camera(*f.cam_args)
    assert (cam.x_pixels(), cam.y_pixels()) == (24, 16)
    for fast in (False, True):
        values, queries = expected(name, which, sky, "image", fast and f.info["local_pool"] == 0, samples=3)
        img, cnt = rayrs_amd.render_lit(f.scene, cam, 3, lights_of(f, which, sky), seed=SEED, sample_chunk=2, fast_traversal=fast, queries=True,
                                        direct=True, mesh=f.mesh)
        assert img.shape == (16, 24, 3) and cnt.shape == (16, 24)
        check((img.reshape(-1, 3), cnt.reshape(-1)), values, queries, 2, (name, which, sky, "image", fast))


@pytest.mark.parametrize("max_bounces", [0, 1])
def test_one_sample_and_the_bounce_bound(max_bounces):
    """S = 1 at max_bounces 50 (with the max_bounces = 1 case), and the bound itself: 0 is +0 and no query, no shadow query
    either; with 1 the shadow sample of the one bounce is traced and credited."""
    f = family("room")
    lights = lights_of(f, "two", True)
    if max_bounces == 0:
        for call, a, b, kw in ((f.scene.radiance, f.o, f.d, {}), (f.scene.irradiance, f.p, f.nrm, dict(bias=1e-4))):
            rad, cnt = call(a, b, samples=3, max_bounces=0, queries=True, lights=lights, direct=True, mesh=f.mesh, **kw)
            assert rad.shape == (len(a), 3) and not bits(rad).any() and not cnt.any()
        return
    for what, call, a, b, kw in (("radiance", f.scene.radiance, f.o, f.d, {}), ("irradiance", f.scene.irradiance, f.p, f.nrm, dict(bias=1e-4))):
        values, queries = expected("room", "two", True, what, samples=1)
        check(call(a, b, samples=1, seed=SEED, queries=True, lights=lights, direct=True, mesh=f.mesh, **kw), values, queries, 0, (what, "S = 1"))
        values, queries = expected("room", "two", True, what, max_bounces=1)
        check(call(a, b, samples=S, seed=SEED, max_bounces=1, sample_chunk=2, queries=True, lights=lights, direct=True, mesh=f.mesh, **kw),
              values, queries, 2, (what, "one bounce"))
        assert queries.max() == (2 if what == "radiance" else 3)


# ------------------------------------------------------------------------------------------------------ the interface

@pytest.mark.parametrize("name", ["room", "mesh1"])
def test_an_empty_group_is_direct_lightings_or_sky_samplings_call_and_a_group_changes_the_answers(name):
    f = family(name)
    empty = f.scene.mesh_lights([])
    lamps = list(f.lists["two" if name == "room" else "lamp"])
    kw = dict(samples=S, seed=SEED, sample_chunk=2, queries=True, direct=True)
    unlit = f.scene.radiance(f.o, f.d, samples=S, seed=SEED, sample_chunk=2, queries=True)
    for fast in (False, True):
        for lights in (lamps, lamps + [SKY], [], [SKY]):
            want = f.scene.radiance(f.o, f.d, lights=lights, fast_traversal=fast, **kw)
            got = f.scene.radiance(f.o, f.d, lights=lights, fast_traversal=fast, mesh=empty, **kw)
            assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1]), (fast, lights)
            # the comparison with the reading is not vacuous: the group changes the bits of the rays that meet a diffuse surface
            grouped = f.scene.radiance(f.o, f.d, lights=lights, fast_traversal=fast, mesh=f.mesh, **kw)
            assert (bits(grouped[0]) != bits(want[0])).any(axis=1).sum() >= 10, (fast, lights)
            want = f.scene.irradiance(f.p, f.nrm, bias=1e-4, lights=lights, fast_traversal=fast, **kw)
            got = f.scene.irradiance(f.p, f.nrm, bias=1e-4, lights=lights, fast_traversal=fast, mesh=empty, **kw)
            assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1]), (fast, lights)
    got = f.scene.radiance(f.o, f.d, lights=[], mesh=empty, **kw)
    assert np.array_equal(bits(got[0]), bits(unlit[0])) and np.array_equal(got[1], unlit[1])
    cam = rayrs_amd.Camera(*f.cam_args)
    for lights in (lamps, lamps + [SKY]):
        want = rayrs_amd.render_lit(f.scene, cam, 3, lights, seed=SEED, sample_chunk=2, queries=True, direct=True)
        got = rayrs_amd.render_lit(f.scene, cam, 3, lights, seed=SEED, sample_chunk=2, queries=True, direct=True, mesh=empty)
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1])
    empty.close()
    with pytest.raises(ValueError):
        f.scene.radiance(f.o, f.d, lights=lamps, mesh=f.mesh)   # (a group is a light of DIRECT lighting)


def test_the_comparisons_are_not_vacuous():
    """From the reading alone, over the default walk's paths of the tests above: the group is drawn, credited, blocked and
    skipped, listed triangles are met with and without a weight, and unlisted emissive triangles sit beside them."""
    for name, which, sky in CASES:
        expected(name, which, sky, "radiance"), expected(name, which, sky, "irradiance")
    for name in ("room", "mesh1"):
        t = family(name).tally
        print(name, t)
        assert t["group_credited"] >= 100 and t["group_skipped_ndl"] >= 10, (name, t)
        assert t["group_blocked_unlisted"] + t["group_blocked_listed"] >= 10, (name, t)
        assert t["met_listed_weighted"] >= 10 and t["met_listed_unweighted"] >= 10, (name, t)
        assert t["lamp_credited"] >= 100 and t["sky_credited"] >= 100, (name, t)
    room, mesh1 = family("room").tally, family("mesh1").tally
    assert room["group_blocked_listed"] >= 1 and room["group_blocked_lamp"] >= 1 and room["lamp_met_listed"] >= 1 and room["sky_met_listed"] >= 1
    assert mesh1["met_unlisted_emissive_triangle"] >= 10 and room["met_unlisted_emissive_triangle"] >= 1


def test_a_slice_with_its_index_base_is_the_slice_of_the_whole():
    f = family("mesh1")
    kw = dict(samples=S, seed=SEED, sample_chunk=2, queries=True, lights=lights_of(f, "lamp", True), direct=True, mesh=f.mesh)
    rad, cnt = f.scene.radiance(f.o, f.d, **kw)
    n = len(f.o)
    for a, b in ((0, 1), (1, 70), (70, 191), (191, n)):
        r, c = f.scene.radiance(f.o[a:b], f.d[a:b], index_base=a, **kw)
        assert np.array_equal(c, cnt[a:b]) and np.array_equal(bits(r), bits(rad[a:b])), (a, b)
    irr, icnt = f.scene.irradiance(f.p, f.nrm, bias=1e-4, **kw)
    r, c = f.scene.irradiance(f.p[7:140], f.nrm[7:140], bias=1e-4, index_base=7, **kw)
    assert np.array_equal(c, icnt[7:140]) and np.array_equal(bits(r), bits(irr[7:140]))
    for call in (f.scene.radiance, f.scene.irradiance):
        r0, c0 = call(np.zeros((0, 3)), np.zeros((0, 3)), samples=3, queries=True, lights=[], direct=True, mesh=f.mesh)
        assert r0.shape == (0, 3) and c0.shape == (0,)


def test_two_handles_on_one_scene_each_give_their_own_bits_and_closing_one_leaves_the_others():
    f = family("mesh1")
    other = f.scene.mesh_lights(f.tris[::2])
    kw = dict(samples=S, seed=SEED, sample_chunk=2, queries=True, lights=lights_of(f, "lamp", False), direct=True)
    a0 = f.scene.radiance(f.o, f.d, mesh=f.mesh, **kw)
    b0 = f.scene.radiance(f.o, f.d, mesh=other, **kw)
    assert (bits(a0[0]) != bits(b0[0])).any()
    for _ in range(2):
        a = f.scene.radiance(f.o, f.d, mesh=f.mesh, **kw)
        b = f.scene.radiance(f.o, f.d, mesh=other, **kw)
        assert np.array_equal(bits(a[0]), bits(a0[0])) and np.array_equal(a[1], a0[1])
        assert np.array_equal(bits(b[0]), bits(b0[0])) and np.array_equal(b[1], b0[1])
    other.close()
    a = f.scene.radiance(f.o, f.d, mesh=f.mesh, **kw)
    assert np.array_equal(bits(a[0]), bits(a0[0])) and np.array_equal(a[1], a0[1])
    with pytest.raises(ValueError):
        f.scene.radiance(f.o, f.d, mesh=other, **kw)
    # a handle of another scene is refused
    with pytest.raises(rayrs_amd._ffi.RayrsError) as e:
        f.scene.radiance(f.o, f.d, mesh=family("room").mesh, **kw)
    assert e.value.status == -1


def test_device_tensors_on_a_stream_give_the_host_paths_bits():
    """tests/_mesh_torch_child.py, in a process of its own (torch has to be imported before the library is loaded)."""
    pytest.importorskip("torch")
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_mesh_torch_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "device path ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_a_render_and_a_direct_call_are_the_same_before_and_after_a_batch_of_mesh_calls():
    f = family("mesh1")
    cam = rayrs_amd.Camera(*f.cam_args)
    lamps = list(f.lists["lamp"])
    before, st0 = rayrs_amd.render(f.scene, cam, 4, out_f64=True)
    direct0 = f.scene.radiance(f.o, f.d, samples=S, lights=lamps, direct=True)
    for fast in (False, True):
        f.scene.radiance(f.o, f.d, samples=S, sample_chunk=2, fast_traversal=fast, lights=lamps + [SKY], direct=True, mesh=f.mesh)
        f.scene.irradiance(f.p, f.nrm, samples=8, bias=1e-4, fast_traversal=fast, lights=[], direct=True, mesh=f.mesh)
        rayrs_amd.render_lit(f.scene, cam, 2, [SKY], fast_traversal=fast, direct=True, mesh=f.mesh)
    after, st1 = rayrs_amd.render(f.scene, cam, 4, out_f64=True)
    direct1 = f.scene.radiance(f.o, f.d, samples=S, lights=lamps, direct=True)
    assert before.tobytes() == after.tobytes() and direct0.tobytes() == direct1.tobytes()
    assert st0["rays"] == st1["rays"] and st0["paths"] == st1["paths"]
