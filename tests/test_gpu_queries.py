"""Ray queries (include/rayrs_hip.h RAY QUERIES) on the GPU, bit for bit against the second reading of geometry.rs and bvh.rs
(tests/_geometry_reading.py): its scenes, its seeded ray families (40,000 to 120,000 rays a scene, no multiple of 256) and its
answers, with G.T0, G.T1 as z_near, z_far.

  * closest hit: object and the bits of t as the reading's and as rayrs_test_intersect's, the normal as tests/_features.py's
    object table gives it at the position FEATURES forms;
  * occlusion on the default walk: `the reading finds a hit and t < t_max`, for t_max families that pin the strict `<`, the
    tie, NaN, zero and negative bounds;
  * occlusion on the fast walk's tree: the same against the oracle's walk over that tree with nothing culled;
  * more than 2^20 rays (several launches), one ray, no ray; the traversal stacks in HBM; device tensors on a stream; and a
    render before and after a batch of queries.

Every test first asserts at least 10,000 hits and 10,000 misses, so neither verdict goes untested."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import _features as F
import _geometry_reading as G
import _oracle
import rayrs_amd
from rayrs_amd import _ffi, scenes
from test_gpu_geometry_reading import HDRI, bits, device_scene, reading, scene_rays
from test_gpu_geometry_reading import intersect as selftest_intersect

pytestmark = pytest.mark.gpu

MISS = 0xFFFFFFFF
CLOSEST = [(s, "sah1000") for s in ("mesh1280_light", "floor_spheres", "soup", "degenerate", "ties", "near_far_t0", "near_far_t1")] + \
          [("mesh1280_light", "midpoint"), ("soup", "midpoint")]
IDS = [f"{s}-{h}" for s, h in CLOSEST]
FAST = ["mesh1280_light", "soup"]


def both_verdicts(robj):
    assert (robj >= 0).sum() >= 10000 and (robj < 0).sum() >= 10000, (int((robj >= 0).sum()), int((robj < 0).sum()))


def want_object(robj):
    return np.where(robj >= 0, robj, MISS).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def expected_normals(scene, heur):
    """object_table(objs)[object] at the hit position as FEATURES forms it (hit_position: o + d * t), +0 on a miss."""
    rays, _ = scene_rays(scene)
    rt, robj = reading(scene, heur)
    out = np.zeros((len(rt), 3))
    with np.errstate(all="ignore"):
        table = F.object_table(G.SCENES[scene]())   # (a degenerate triangle's normal is NaN; no ray hits one)
        p = G.point(G.vec(rays.o), G.vec(rays.d), rt)
        for k in np.unique(robj[robj >= 0]):
            m = robj == k
            nx, ny, nz = table[int(k)][0](G.take(p, m))
            out[m, 0], out[m, 1], out[m, 2] = nx, ny, nz
    return out


def t_max_families(rt, robj):
    """name -> t_max per ray (None: the argument left out); t* is the expected closest t (0 on a miss)."""
    n, hit = len(rt), robj >= 0
    median = float(np.median(rt[hit]))
    return {"none": None, "inf": np.full(n, np.inf), "t_star": rt.copy(), "next_after_t_star": np.nextafter(rt, np.inf),
            "half_t_star": 0.5 * rt, "twice_t_star": 2.0 * rt, "nan": np.full(n, np.nan), "zero": np.zeros(n),
            "negative": np.full(n, -1.0), "median_hit_t": np.full(n, median)}


def want_occluded(rt, robj, t_max):
    if t_max is None:
        return robj >= 0
    with np.errstate(all="ignore"):
        return (robj >= 0) & (rt < t_max)


def assert_occluded(sc, rays, rt, robj, fast, what):
    hit = robj >= 0
    for name, t_max in t_max_families(rt, robj).items():
        got = sc.occluded(rays.o, rays.d, t_max, fast_traversal=fast)
        want = want_occluded(rt, robj, t_max)
        assert got.dtype == np.bool_ and got.shape == want.shape
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, (what, name, len(bad), [(int(i), int(robj[i]), float(rt[i])) for i in bad[:5]])
        assert not got[~hit].any()
        if name in ("t_star", "half_t_star", "nan", "zero", "negative"):
            assert not got.any(), (what, name)
        if name in ("none", "inf", "next_after_t_star", "twice_t_star"):
            assert got[hit].all(), (what, name)  # next_after_t_star: the strict `<`, and on `ties` the tie


# ------------------------------------------------------------------------------------------------------ closest hit

@pytest.mark.parametrize("scene,heur", CLOSEST, ids=IDS)
def test_closest_hit_is_the_readings_and_the_self_tests(scene, heur):
    rays, _ = scene_rays(scene)
    rt, robj = reading(scene, heur)
    both_verdicts(robj)
    sc, _ = device_scene(scene, heur)
    t, obj, nrm = sc.intersect(rays.o, rays.d, normals=True)
    assert t.dtype == np.float64 and obj.dtype == np.uint32 and nrm.shape == (len(rt), 3)
    hit = robj >= 0
    assert np.array_equal(obj, want_object(robj))
    assert np.array_equal(bits(t)[hit], bits(rt)[hit]) and (bits(t)[~hit] == 0).all()   # +0 on a miss
    st, sobj = selftest_intersect(sc, rays.o, rays.d)
    assert np.array_equal(obj, want_object(sobj)) and np.array_equal(bits(t), bits(st))
    want = expected_normals(scene, heur)
    bad = np.flatnonzero((bits(nrm) != bits(want)).any(axis=1))
    assert len(bad) == 0, (len(bad), [(int(i), int(robj[i]), nrm[i].tolist(), want[i].tolist()) for i in bad[:5]])
    assert (bits(nrm)[~hit] == 0).all()
    t2, obj2 = sc.intersect(rays.o, rays.d)                                              # normals=False changes nothing else
    assert np.array_equal(bits(t2), bits(t)) and np.array_equal(obj2, obj)


# ------------------------------------------------------------------------------------------------------ occlusion

@pytest.mark.parametrize("scene,heur", CLOSEST, ids=IDS)
def test_occlusion_on_the_default_walk_is_the_closest_hit_verdict(scene, heur):
    rays, _ = scene_rays(scene)
    rt, robj = reading(scene, heur)
    both_verdicts(robj)
    sc, _ = device_scene(scene, heur)
    assert_occluded(sc, rays, rt, robj, False, (scene, heur))


@functools.lru_cache(maxsize=None)
def fast_tree_reading(scene):
    """The oracle's walk over the tree of single primitives behind their own boxes with nothing culled."""
    rays, _ = scene_rays(scene)
    objs = G.SCENES[scene]()
    prod = rayrs_amd.Scene(objs, G.T0, G.T1, G.HEURISTICS["sah1000"], HDRI, device=-1)
    osc = _oracle.OracleScene(objs, G.T0, G.T1, G.HEURISTICS["sah1000"], HDRI).use_walk_tree(prod)
    try:
        _oracle.set_cull_margin(float("inf"))
        return osc.intersect_batch(rays.o, rays.d, G.T0, G.T1, traversal=2, nthreads=16)
    finally:
        _oracle.set_cull_margin(2.0 ** -10)


@pytest.mark.parametrize("scene", FAST)
def test_occlusion_on_the_fast_walks_tree_is_that_trees_verdict(scene):
    rays, _ = scene_rays(scene)
    ft, fobj = fast_tree_reading(scene)
    both_verdicts(fobj)
    sc, _ = device_scene(scene, "sah1000")
    assert_occluded(sc, rays, ft, fobj, True, (scene, "fast"))


# ------------------------------------------------------------------------------------------------------ launches

def test_more_than_a_launch_of_rays_one_ray_and_none():
    """soup's 120,000 rays nine times over: 1,080,000 > 2^20, so the batch takes two launches; then n = 1 and n = 0."""
    rays, _ = scene_rays("soup")
    rt, robj = reading("soup", "sah1000")
    both_verdicts(robj)
    reps = 9
    o, d = np.tile(rays.o, (reps, 1)), np.tile(rays.d, (reps, 1))
    assert len(o) == 1080000 > 1 << 20
    sc, _ = device_scene("soup", "sah1000")
    t, obj, nrm = sc.intersect(o, d, normals=True)
    assert np.array_equal(obj, np.tile(want_object(robj), reps))
    assert np.array_equal(bits(t), np.tile(bits(np.where(robj >= 0, rt, 0.0)), reps))
    assert np.array_equal(bits(nrm), np.tile(bits(expected_normals("soup", "sah1000")), (reps, 1)))
    got = sc.occluded(o, d, np.tile(np.nextafter(rt, np.inf), reps))
    assert np.array_equal(got, np.tile(robj >= 0, reps))
    # one ray: a hit and a miss, each alone
    for i in (int(np.flatnonzero(robj >= 0)[0]), int(np.flatnonzero(robj < 0)[0])):
        t1, obj1, nrm1 = sc.intersect(rays.o[i:i + 1], rays.d[i:i + 1], normals=True)
        assert (bits(t1)[0], obj1[0]) == (bits(t)[i], obj[i]) and np.array_equal(bits(nrm1)[0], bits(nrm)[i])
        assert sc.occluded(rays.o[i:i + 1], rays.d[i:i + 1]).tolist() == [bool(robj[i] >= 0)]
    # none: RAYRS_OK, nothing launched, empty answers
    t0, obj0, nrm0 = sc.intersect(np.zeros((0, 3)), np.zeros((0, 3)), normals=True)
    assert t0.shape == (0,) and obj0.shape == (0,) and nrm0.shape == (0, 3)
    assert sc.occluded(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0)).shape == (0,)
    L, one = sc._L, np.zeros(3)
    assert L.rayrs_scene_intersect(sc._h, one.ctypes.data, one.ctypes.data, 0, 0, one.ctypes.data, one.ctypes.data, None) == 0
    assert L.rayrs_scene_occluded(sc._h, one.ctypes.data, one.ctypes.data, None, 0, 1, one.ctypes.data) == 0
    assert L.rayrs_scene_intersect(sc._h, one.ctypes.data, one.ctypes.data, 0, 0, None, one.ctypes.data, None) == -1


def test_the_stacks_in_hbm_change_nothing():
    """rayrs_lab stack_lds = 2: all but two entries of a lane's stack live in the strip the scene keeps for the queries."""
    rays, _ = scene_rays("mesh5120")
    rt, robj = reading("mesh5120", "sah1000")
    both_verdicts(robj)
    sc, info = device_scene("mesh5120", "sah1000")
    assert info["hot_depth"] > 2 and info["wide_depth"] > 2   # some entries do go to the strip, on either tree
    sc.lab_set(stack_lds=2)
    t, obj = sc.intersect(rays.o, rays.d)
    hit = robj >= 0
    assert np.array_equal(obj, want_object(robj)) and np.array_equal(bits(t)[hit], bits(rt)[hit]) and (bits(t)[~hit] == 0).all()
    for t_max in (None, np.nextafter(rt, np.inf), rt):
        assert np.array_equal(sc.occluded(rays.o, rays.d, t_max), want_occluded(rt, robj, t_max))
    # the fast walk's tree through the same strip: the any-hit verdict with no bound is "the closest-hit query hits"
    ft, fobj = sc.intersect(rays.o, rays.d, fast_traversal=True)
    sc.lab_set()
    ft0, fobj0 = sc.intersect(rays.o, rays.d, fast_traversal=True)
    assert np.array_equal(fobj, fobj0) and np.array_equal(bits(ft), bits(ft0))


def test_device_tensors_on_a_stream_give_the_host_paths_bits():
    """tests/_query_torch_child.py, in a process of its own: torch brings its own copy of the HIP runtime and has to be
    imported before the library is loaded for the two to share one (bench.py imports it first for the same reason); in this
    process the library came first.  The child answers floor_spheres' rays from f64 tensors on the GPU inside a side stream,
    compares them bit for bit with the host path's after a stream sync, and checks the refusals."""
    pytest.importorskip("torch")
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_query_torch_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "device path ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_a_render_is_the_same_before_and_after_a_batch_of_queries():
    cam_args, objs, heur = scenes.mesh_scene(3, area_light=True)
    sc = rayrs_amd.Scene(objs, G.T0, G.T1, heur, HDRI, device=0)
    cam = rayrs_amd.Camera(*scenes.camera_for_resolution(cam_args, 48, 32))
    before, st0 = rayrs_amd.render(sc, cam, 4, out_f64=True)
    rays, _ = scene_rays("mesh1280_light")
    for fast in (False, True):
        sc.intersect(rays.o, rays.d, fast_traversal=fast, normals=True)
        sc.occluded(rays.o, rays.d, fast_traversal=fast)
    after, st1 = rayrs_amd.render(sc, cam, 4, out_f64=True)
    assert before.tobytes() == after.tobytes()
    assert st0["rays"] == st1["rays"] and st0["paths"] == st1["paths"]


def test_the_labs_step_count_shows_the_early_exit():
    """rayrs_lab_query_steps (scripts/ubench/query_bench.py's idle measure): the verdicts are rayrs_scene_occluded's; with a NaN
    t_max no ray stops early, so no ray takes fewer turns than with t_max = inf, a miss takes as many, and some hit takes more."""
    rays, _ = scene_rays("floor_spheres")
    rt, robj = reading("floor_spheres", "sah1000")
    both_verdicts(robj)
    sc, _ = device_scene("floor_spheres", "sah1000")
    n = len(rt)

    def steps(t_max):
        occ, st = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint32)
        _ffi.check(sc._L.rayrs_lab_query_steps(sc._h, rays.o.ctypes.data, rays.d.ctypes.data, None if t_max is None else t_max.ctypes.data,
                                               n, 0, occ.ctypes.data, st.ctypes.data), "rayrs_lab_query_steps")
        return occ.astype(bool), st

    occ_inf, st_inf = steps(None)
    occ_nan, st_nan = steps(np.full(n, np.nan))
    hit = robj >= 0
    assert np.array_equal(occ_inf, hit) and not occ_nan.any()
    assert (st_nan >= st_inf).all() and np.array_equal(st_nan[~hit], st_inf[~hit]) and (st_nan[hit] > st_inf[hit]).any()
    assert sc._L.rayrs_lab_query_steps(sc._h, rays.o.ctypes.data, rays.d.ctypes.data, None, n, 0, occ_inf.ctypes.data, None) == -1
