"""Radiance queries (include/rayrs_hip.h RADIANCE QUERY, IRRADIANCE) on the GPU, bit for bit and count for count against the
plain-Python reading of the operation (tests/_radiance.py), whose paths are the oracle's radiance() on the caller's ray with the
key and the draw the header names.  The rays are the oracle camera's primary rays with the sample-0 key of primary seed 77, over
the whole image; S = 5 with sample_chunk 0 and 2.

The kernel shades, refills and walks a wave's lanes side by side and hands items out from one device-wide cursor, so besides
the parity there are the paths that run to the bounce budget, the shapes where that schedule can go wrong, every threshold of
the wave, batches cut in pieces and across launches, device tensors on a stream, and a render before and after."""
import functools
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import _ao
import _oracle
import _radiance
import rayrs_amd
from rayrs_amd import procedural, scenes
from rayrs_amd.api import Material
from test_gpu_deep_paths import HDRI as ROOM_HDRI, Z_NEAR as ROOM_Z_NEAR, hot_room, white_room

pytestmark = pytest.mark.gpu

HDRI = procedural.make_hdri(128, 64)
Z_NEAR, Z_FAR = 1e-6, 1e6
S = 5
SEED = 0x5EED
PRIMARY_SEED = 77
FAMILIES = {
    "material_test": (scenes.material_test, 48, 10, Z_NEAR, "std"),
    "frosted_glass": (scenes.cook_torrance_spheres_frosted_glass, 40, 16, Z_NEAR, "std"),
    "mesh3_light": (lambda: scenes.mesh_scene(3, Material.LambertianDiffuse((0.8, 0.8, 0.8)), area_light=True), 32, 24, Z_NEAR, "std"),
    "mesh4": (lambda: scenes.mesh_scene(4), 32, 24, Z_NEAR, "std"),
    "white_room": (white_room, 16, 12, ROOM_Z_NEAR, "room"),
    "hot_room": (hot_room, 16, 12, ROOM_Z_NEAR, "room"),
}


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def primary_rays(cam_args, w, h):
    """Sample 0's primary ray of every pixel, in image order: (origins, directions), (h * w, 3) each."""
    ocam = _oracle.OracleCamera(*scenes.camera_for_resolution(cam_args, w, h))
    assert (ocam.x_pixels(), ocam.y_pixels()) == (w, h)
    o, d = np.zeros((h * w, 3)), np.zeros((h * w, 3))
    for r in range(h):
        for c in range(w):
            o[r * w + c], d[r * w + c], _ = ocam.primary_ray(h - r, w - c, _ao.path_key(PRIMARY_SEED, r * w + c, 0))
    o.setflags(write=False), d.setflags(write=False)
    return o, d


@functools.lru_cache(maxsize=None)
def family(name):
    """The family's objects, its rays, its scene on the device, and two oracle scenes: the reference's walk, and (fast) the
    product's fast walk on the product's records (the recipe of tests/test_gpu_render.py)."""
    make, w, h, z_near, env = FAMILIES[name]
    cam_args, objs, heur = make()
    hdri = HDRI if env == "std" else ROOM_HDRI
    o, d = primary_rays(cam_args, w, h)
    scene = rayrs_amd.Scene(objs, z_near, Z_FAR, heur, hdri, device=0)
    osc = _oracle.OracleScene(objs, z_near, Z_FAR, heur, hdri)
    fast = _oracle.OracleScene(objs, z_near, Z_FAR, heur, hdri).use_product_walk(scene, fast=True)
    return SimpleNamespace(name=name, objs=objs, heur=heur, hdri=hdri, z_near=z_near, cam_args=cam_args, w=w, h=h, o=o, d=d,
                           scene=scene, osc=osc, fast=fast, info=scene.info())


@functools.lru_cache(maxsize=None)
def expected_paths(name, max_bounces, fast=False, samples=S, first=0, n=None):
    """The oracle's paths of the family's rays first .. first + n - 1 with index_base = first: (values, queries)."""
    f = family(name)
    last = None if n is None else first + n
    return _radiance.radiance_paths(f.fast if fast else f.osc, f.o[first:last], f.d[first:last], samples, max_bounces, SEED, first,
                                    traversal=2 if fast else 0)


def check(got, values, queries, chunk, what):
    rad, cnt = got
    want_rad, want_cnt = _radiance.answers(values, queries, chunk)
    assert rad.dtype == np.float64 and cnt.dtype == np.uint32 and rad.shape == want_rad.shape and cnt.shape == want_cnt.shape, what
    bad = np.flatnonzero(cnt != want_cnt)
    assert len(bad) == 0, (what, "queries", len(bad), [(int(i), int(cnt[i]), int(want_cnt[i])) for i in bad[:5]])
    bad = np.flatnonzero((bits(rad) != bits(want_rad)).any(axis=1))
    assert len(bad) == 0, (what, "radiance", len(bad), [(int(i), rad[i].tolist(), want_rad[i].tolist()) for i in bad[:3]])
    assert np.isfinite(rad).all(), what
    return want_rad, want_cnt


def differing(values, queries):
    """How many rays' means differ in bits between sample_chunk 0 and 2."""
    return int((bits(_radiance.answers(values, queries, 0)[0]) != bits(_radiance.answers(values, queries, 2)[0])).any(axis=1).sum())


# ------------------------------------------------------------------------------------------------------ parity

PARITY = [("material_test", 50), ("frosted_glass", 50), ("frosted_glass", 3), ("mesh3_light", 50), ("mesh4", 50)]


@pytest.mark.parametrize("name,max_bounces", PARITY, ids=[f"{n}-{b}" for n, b in PARITY])
def test_radiance_and_queries_are_the_oracles(name, max_bounces):
    f = family(name)
    values, queries = expected_paths(name, max_bounces)
    n = len(f.o)
    nonzero = int((_radiance.answers(values, queries, 0)[0] != 0.0).any(axis=1).sum())
    deep = int((queries >= 4).sum())
    print(name, max_bounces, "rays", n, "paths with >= 4 queries", deep, "non-zero rays", nonzero, "differ c=0 / c=2", differing(values, queries))
    # the conditions that keep the comparison from being vacuous, from the oracle alone
    if name == "material_test":
        first = np.array([f.osc.intersect(f.o[i], f.d[i], f.z_near, Z_FAR)[0] for i in range(n)])
        per_object = [int((first == k).sum()) for k in range(8)]
        print("first hits per object", per_object, "misses", int((first < 0).sum()))
        assert n == 480 and min(per_object) >= 10 and (first < 0).sum() >= 100
        assert deep >= 50 and nonzero >= 400 and differing(values, queries) >= 10
    elif name == "frosted_glass":
        assert n * S == 3200
        assert deep >= 150 if max_bounces == 50 else queries.max() <= 3
    elif name == "mesh3_light":
        assert n == 768 and deep >= 40 and nonzero >= 600 and differing(values, queries) >= 40
    for chunk in (0, 2):
        check(f.scene.radiance(f.o, f.d, samples=S, max_bounces=max_bounces, seed=SEED, sample_chunk=chunk, queries=True), values, queries,
              chunk, (name, max_bounces, chunk))
    fvalues, fqueries = expected_paths(name, max_bounces, fast=True)
    for chunk in (0, 2):
        check(f.scene.radiance(f.o, f.d, samples=S, max_bounces=max_bounces, seed=SEED, sample_chunk=chunk, fast_traversal=True, queries=True),
              fvalues, fqueries, chunk, (name, max_bounces, chunk, "fast"))


@pytest.mark.parametrize("name", ["white_room", "hot_room"])
def test_paths_that_run_to_the_bounce_budget(name):
    """Closed rooms whose every scattering weight is exactly one: the roulette never fires and every path makes max_bounces
    queries.  hot_room is a scene of the streaming route with a hot group."""
    f = family(name)
    budget = 200
    values, queries = expected_paths(name, budget)
    assert len(f.o) == 192 and (queries == budget).all()
    assert (_radiance.answers(values, queries, 0)[0] != 0.0).any(axis=1).all() and differing(values, queries) >= 20
    if name == "hot_room":
        assert f.info["hot_count"] > 0 and f.info["local_pool"] == 0
    for fast in (False, True):
        v, q = expected_paths(name, budget, fast=fast)
        for chunk in (0, 2):
            check(f.scene.radiance(f.o, f.d, samples=S, max_bounces=budget, seed=SEED, sample_chunk=chunk, fast_traversal=fast, queries=True),
                  v, q, chunk, (name, chunk, fast))


# ------------------------------------------------------------------------------------------------------ irradiance

def floor_grid():
    x = np.linspace(-4.0, 4.0, 24)
    p = np.array([(xi, 0.0, zi) for zi in x for xi in x])
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def expected_irradiance(name, ny, bias, max_bounces, fast=False):
    f = family(name)
    p = floor_grid()
    return _radiance.irradiance_paths(f.fast if fast else f.osc, p, np.tile((0.0, ny, 0.0), (len(p), 1)), 8, bias, max_bounces, SEED,
                                      traversal=2 if fast else 0)


@pytest.mark.parametrize("name,max_bounces", [("mesh3_light", 50), ("hot_room", 100)])
def test_irradiance_at_floor_points_is_the_oracles(name, max_bounces):
    """A 24 x 24 grid of floor points with the normal (0, 1, 0) and, used as given, (0, 2, 0); bias 1e-4 and 0.  In hot_room a
    lane's direction-making meets long walks."""
    f = family(name)
    p = floor_grid()
    for ny in (1.0, 2.0):
        nrm = np.tile((0.0, ny, 0.0), (len(p), 1))
        for bias in (1e-4, 0.0):
            values, queries = expected_irradiance(name, ny, bias, max_bounces)
            if name == "mesh3_light":
                print(name, ny, bias, "queries a path: mean", float(queries.mean()), "max", int(queries.max()))
                assert len(p) == 576 and (_radiance.answers(values, queries, 0)[0] != 0.0).any(axis=1).all() and queries.max() >= 4
            else:
                assert queries.max() == max_bounces
            for chunk in (0, 3):
                check(f.scene.irradiance(p, nrm, samples=8, bias=bias, max_bounces=max_bounces, seed=SEED, sample_chunk=chunk, queries=True),
                      values, queries, chunk, (name, ny, bias, chunk))
    values, queries = expected_irradiance(name, 1.0, 1e-4, max_bounces, fast=True)
    check(f.scene.irradiance(p, np.tile((0.0, 1.0, 0.0), (len(p), 1)), samples=8, bias=1e-4, max_bounces=max_bounces, seed=SEED, sample_chunk=3,
                             fast_traversal=True, queries=True), values, queries, 3, (name, "fast"))


# ------------------------------------------------------------------------------------------------------ the schedule

def schedule_start():
    """The first of material_test's rays one of whose five paths makes four queries or more (and that leaves 257 rays behind it):
    index_base keeps the parity test's keys, so a lone ray's many samples are not all one short path."""
    _, queries = expected_paths("material_test", 50)
    return int(min(np.flatnonzero((queries >= 4).any(axis=1))[0], len(queries) - 257))


@pytest.mark.parametrize("n,samples,chunk", [(1, 1, 0), (1, 257, 4), (1, 4096, 4), (3, 64, 0), (70, 67, 5), (257, 1, 0)])
def test_shapes_where_the_schedule_can_go_wrong(n, samples, chunk):
    """One item, a lone ray's chunks spread over many waves and workgroups (1,024 items from one cursor), fewer items than a
    wave, chunks that do not divide S, more rays than a workgroup has lanes."""
    f = family("material_test")
    a = schedule_start()
    values, queries = expected_paths("material_test", 50, samples=samples, first=a, n=n)
    got = f.scene.radiance(f.o[a:a + n], f.d[a:a + n], samples=samples, seed=SEED, index_base=a, sample_chunk=chunk, queries=True)
    check(got, values, queries, chunk, (n, samples, chunk))
    if samples >= 64:
        assert queries.max() >= 4 and queries.min() <= 2


def knob_settings():
    return [(r, s, l) for r in (1, 0, 64) for s in (1, 0, 64) for l in (1, 0, 64)]


@pytest.mark.parametrize("name,max_bounces,stack_lds", [("material_test", 50, 0), ("hot_room", 200, 0), ("mesh4", 50, 2)],
                         ids=["material_test", "hot_room", "mesh4-stacks_in_hbm"])
def test_every_threshold_gives_the_same_bits(name, max_bounces, stack_lds):
    """rayrs_lab_radiance_tuning: each of refill_below, shade_at and leaf_min at 1, at its default and at 64, all 27 settings, on
    both walks; (1, 64, .) is the kernel that refills only an empty wave and shades only when no lane walks.  On mesh4 with
    stack_lds = 2 all but two entries of a lane's stack live in the strip the scene keeps for the queries.  Mandatory for any
    change of the scheduler."""
    f = family(name)
    if stack_lds:
        assert f.info["wide_depth"] > stack_lds and (f.info["hot_depth"] if f.info["hot_count"] else f.info["gate_depth"]) > stack_lds
        f.scene.lab_set(stack_lds=stack_lds)
    p = floor_grid()[::7]
    nrm = np.tile((0.0, 1.0, 0.0), (len(p), 1))
    try:
        for fast in (False, True):
            values, queries = expected_paths(name, max_bounces, fast=fast)
            first = None
            for knobs in knob_settings():
                f.scene.lab_radiance_tuning(*knobs)
                check(f.scene.radiance(f.o, f.d, samples=S, max_bounces=max_bounces, seed=SEED, sample_chunk=2, fast_traversal=fast, queries=True),
                      values, queries, 2, (name, fast, knobs))
                irr = f.scene.irradiance(p, nrm, samples=6, bias=1e-4, max_bounces=max_bounces, seed=SEED, sample_chunk=4, fast_traversal=fast,
                                         queries=True)
                if first is None:
                    first = irr
                assert np.array_equal(bits(irr[0]), bits(first[0])) and np.array_equal(irr[1], first[1]), (name, fast, knobs)
    finally:
        f.scene.lab_radiance_tuning(0, 0, 0)
        if stack_lds:
            f.scene.lab_set()
    assert f.scene._L.rayrs_lab_radiance_tuning(f.scene._h, 65, 0, 0) == -1


def lab_turns(scene, irradiance, a, b, samples, max_bounces, chunk, bias, index_base, fast):
    """rayrs_lab.h rayrs_lab_radiance_turns: the kernel's instance that also counts its turns.  (queries, turns)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    queries, turns = np.zeros(len(a), dtype=np.uint32), np.zeros(3, dtype=np.uint64)
    rayrs_amd._ffi.check(scene._L.rayrs_lab_radiance_turns(scene._h, int(irradiance), a.ctypes.data, b.ctypes.data, len(a), samples, max_bounces,
                                                          chunk, bias, SEED, index_base, int(fast), queries.ctypes.data, turns.ctypes.data),
                         "rayrs_lab_radiance_turns")
    return queries, turns


def test_the_turn_counting_instance_makes_the_oracles_queries():
    """The lab's instance of the kernel answers with query counts and three turn counters, no radiance: the counts are the
    oracle's, ray for ray, on 130 rays (two full waves and two lanes) and 130 points, S = 5 in chunks of 2 (three chunks, the last
    short), max_bounces 4.  The counters: a shade turn of a lane ends exactly one ray, so the lane-turns spent shading are the
    queries; a lane walks or is shaded at most once in a wave's turn, so both together are at most 64 x the waves' turns."""
    f = family("material_test")
    a, n, samples, chunk, bounces = schedule_start(), 130, 5, 2, 4
    for fast in (False, True):
        values, queries = expected_paths("material_test", bounces, fast=fast, samples=samples, first=a, n=n)
        want = _radiance.answers(values, queries, chunk)[1]
        assert (queries == bounces).sum() >= 30 and (queries == 1).sum() >= 200   # (paths cut by the budget, and rays that miss)
        got, turns = lab_turns(f.scene, False, f.o[a:a + n], f.d[a:a + n], samples, bounces, chunk, 0.0, a, fast)
        assert np.array_equal(got, want), (fast, np.flatnonzero(got != want)[:5])
        assert int(turns[2]) == int(want.sum()) and turns[0] % 64 == 0 and turns[1] + turns[2] <= turns[0], (fast, turns)
    p = floor_grid()[:n]
    nrm = np.tile((0.0, 1.0, 0.0), (n, 1))
    values, queries = _radiance.irradiance_paths(f.osc, p, nrm, samples, 1e-4, bounces, SEED)
    want = _radiance.answers(values, queries, chunk)[1]
    got, turns = lab_turns(f.scene, True, p, nrm, samples, bounces, chunk, 1e-4, 0, False)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:5]
    assert int(turns[2]) == int(want.sum()) and turns[0] % 64 == 0 and turns[1] + turns[2] <= turns[0], turns
    # and the same counts from the kernel that does not count turns
    assert np.array_equal(f.scene.irradiance(p, nrm, samples=samples, bias=1e-4, max_bounces=bounces, seed=SEED, sample_chunk=chunk, queries=True)[1], got)


# ------------------------------------------------------------------------------------------------------ slices, launches, outputs

def test_a_slice_with_its_index_base_is_the_slice_of_the_whole_also_across_launches():
    f = family("material_test")
    kw = dict(samples=S, seed=SEED, sample_chunk=2, queries=True)
    rad, cnt = f.scene.radiance(f.o, f.d, **kw)
    n = len(f.o)
    for a, b in ((0, 1), (1, 130), (130, 401), (401, n)):
        r, c = f.scene.radiance(f.o[a:b], f.d[a:b], index_base=a, **kw)
        assert np.array_equal(c, cnt[a:b]) and np.array_equal(bits(r), bits(rad[a:b])), (a, b)
    assert not np.array_equal(bits(f.scene.radiance(f.o[130:401], f.d[130:401], index_base=0, **kw)[0]), bits(rad[130:401]))   # (other keys)
    # S = 1: an item a ray and 2^20 of them a launch; the rays 2,185 times over is more than that
    reps = 2185
    big_o, big_d = np.tile(f.o, (reps, 1)), np.tile(f.d, (reps, 1))
    m = len(big_o)
    assert 1 << 20 < m < (1 << 20) + 1000
    kw1 = dict(samples=1, seed=SEED, queries=True)
    rad, cnt = f.scene.radiance(big_o, big_d, **kw1)
    pieces = [f.scene.radiance(big_o[a:b], big_d[a:b], index_base=a, **kw1) for a, b in ((0, 300001), (300001, 1048577), (1048577, m))]
    assert np.array_equal(np.concatenate([c for _, c in pieces]), cnt)
    assert np.array_equal(bits(np.concatenate([r for r, _ in pieces])), bits(rad))
    values, queries = expected_paths("material_test", 50, samples=1)
    want_rad, want_cnt = _radiance.answers(values, queries, 0)
    assert np.array_equal(cnt[:n], want_cnt) and np.array_equal(bits(rad[:n]), bits(want_rad))
    assert np.array_equal(cnt[-n:] > 0, want_cnt > 0) and not np.array_equal(bits(rad[-n:]), bits(want_rad))   # (other keys: no copy)
    # none: RAYRS_OK, nothing launched, empty answers; no bounce: +0 and no query
    for call in (f.scene.radiance, f.scene.irradiance):
        r0, c0 = call(np.zeros((0, 3)), np.zeros((0, 3)), samples=3, queries=True)
        assert r0.shape == (0, 3) and c0.shape == (0,)
        r0, c0 = call(f.o[:70], f.d[:70], samples=3, max_bounces=0, queries=True)
        assert not bits(r0).any() and not c0.any() and r0.shape == (70, 3)


def test_one_output_alone_is_the_same_output():
    f = family("mesh3_light")
    L, n = f.scene._L, len(f.o)
    o, d = np.ascontiguousarray(f.o), np.ascontiguousarray(f.d)
    both = f.scene.radiance(o, d, samples=S, seed=SEED, sample_chunk=2, queries=True)
    rad, cnt = np.zeros((n, 3)), np.zeros(n, dtype=np.uint32)
    assert L.rayrs_scene_radiance(f.scene._h, o.ctypes.data, d.ctypes.data, n, S, 50, 2, SEED, 0, 0, rad.ctypes.data, None) == 0
    assert L.rayrs_scene_radiance(f.scene._h, o.ctypes.data, d.ctypes.data, n, S, 50, 2, SEED, 0, 0, None, cnt.ctypes.data) == 0
    assert np.array_equal(bits(rad), bits(both[0])) and np.array_equal(cnt, both[1])
    p = np.ascontiguousarray(floor_grid())
    nrm = np.tile((0.0, 1.0, 0.0), (len(p), 1))
    both = f.scene.irradiance(p, nrm, samples=8, bias=1e-4, seed=SEED, queries=True)
    rad, cnt = np.zeros((len(p), 3)), np.zeros(len(p), dtype=np.uint32)
    assert L.rayrs_scene_irradiance(f.scene._h, p.ctypes.data, nrm.ctypes.data, len(p), 8, 50, 0, 1e-4, SEED, 0, 0, rad.ctypes.data, None) == 0
    assert L.rayrs_scene_irradiance(f.scene._h, p.ctypes.data, nrm.ctypes.data, len(p), 8, 50, 0, 1e-4, SEED, 0, 0, None, cnt.ctypes.data) == 0
    assert np.array_equal(bits(rad), bits(both[0])) and np.array_equal(cnt, both[1])


def test_device_tensors_on_a_stream_give_the_host_paths_bits():
    """tests/_radiance_torch_child.py, in a process of its own (torch has to be imported before the library is loaded)."""
    pytest.importorskip("torch")
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_radiance_torch_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "device path ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_a_render_is_the_same_before_and_after_a_batch_of_radiance_calls():
    f = family("mesh3_light")
    cam = rayrs_amd.Camera(*scenes.camera_for_resolution(f.cam_args, 48, 32))
    before, st0 = rayrs_amd.render(f.scene, cam, 4, out_f64=True)
    p = floor_grid()
    nrm = np.tile((0.0, 1.0, 0.0), (len(p), 1))
    for fast in (False, True):
        f.scene.radiance(f.o, f.d, samples=S, sample_chunk=2, fast_traversal=fast)
        f.scene.irradiance(p, nrm, samples=8, bias=1e-4, fast_traversal=fast)
    after, st1 = rayrs_amd.render(f.scene, cam, 4, out_f64=True)
    assert before.tobytes() == after.tobytes()
    assert st0["rays"] == st1["rays"] and st0["paths"] == st1["paths"]
