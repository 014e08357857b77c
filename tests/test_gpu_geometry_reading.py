"""The kernels' ray queries against the second reading of geometry.rs and bvh.rs (tests/_geometry_reading.py), bit for bit:
the object of every ray, the bits of t where there is a hit, on every scene and ray family of
tests/test_second_reading_of_geometry_rs.py under three builders.  Two routes:

  * rayrs_test_intersect: one lane per query, the hot group and then the plain record and leaf steps (kernels.hip);
  * rayrs_test_trace: the kernels a render answers its queries with -- the rays go into pool slots as the kernels that make
    rays leave them (finish_rays' pre-test of the hot group and the first record, on a scene with one) and through the
    traversal kernel's rounds, with its LDS record cache, window lists and leaf queue (wavefront.hip).

On a compact and an f64 scene both walks run with the record test (device_path.h trav_record_test) reading every record from HBM
and reading the first from LDS.  On the hot-group scenes the trace runs again with the whole gate tree (rayrs_lab hot_group), with each leaf-queue setting of
test_gpu_hot_group.test_leaf_groups_set_aside_in_any_order_change_nothing, and through a pool of 1024 slots."""
import functools

import numpy as np
import pytest

import _geometry_reading as G
import rayrs_amd
from rayrs_amd import _ffi, procedural

pytestmark = pytest.mark.gpu

HDRI = procedural.make_hdri(8, 4)
HOT_SCENES = ("mesh1280_light", "mesh5120", "degenerate", "floor_spheres")
LEAF_QUEUE = [dict(leaf_min=64, leaf_wait=64), dict(leaf_min=64, leaf_wait=64, refill_min=64, stack_lds=2),
              dict(leaf_min=1, leaf_wait=1), dict(leaf_min=64, leaf_wait=1, refill_min=1)]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def scene_rays(scene):
    return G.scene_rays(scene)


@functools.lru_cache(maxsize=None)
def reading(scene, heur):
    rays, spans = scene_rays(scene)
    r = G.Reading(G.SCENES[scene](), G.HEURISTICS[heur])
    t, obj = r.intersect(rays.o, rays.d)
    return t, obj


def intersect(scene, o, d):
    t, obj = np.zeros(len(o)), np.zeros(len(o), dtype=np.int64)
    _ffi.check(scene._L.rayrs_test_intersect(scene._h, o.ctypes.data, d.ctypes.data, len(o), 1, t.ctypes.data,
                                             obj.ctypes.data), "rayrs_test_intersect")
    return t, obj


def trace(scene, o, d, exact=1):
    t, obj, answered = np.zeros(len(o)), np.zeros(len(o), dtype=np.int64), np.zeros(1, dtype=np.uint64)
    _ffi.check(scene._L.rayrs_test_trace(scene._h, o.ctypes.data, d.ctypes.data, len(o), exact, t.ctypes.data,
                                         obj.ctypes.data, answered.ctypes.data), "rayrs_test_trace")
    return t, obj, int(answered[0])


def assert_same(got, want, what):
    (t, obj), (rt, robj) = got, want
    bad = np.flatnonzero((obj != robj) | ((robj >= 0) & (bits(t) != bits(rt))))
    assert len(bad) == 0, (what, len(bad), [(int(i), int(obj[i]), int(robj[i]), float(t[i]), float(rt[i])) for i in bad[:5]])


def device_scene(scene, heur):
    sc = rayrs_amd.Scene(G.SCENES[scene](), G.T0, G.T1, G.HEURISTICS[heur], HDRI, device=0)
    info = sc.info()
    if scene.startswith("mesh"):
        assert info["compact"] == 1
    if scene in ("soup", "grid_soup"):
        assert info["compact"] == 0
    assert (info["hot_count"] >= 1) == (scene in HOT_SCENES)
    return sc, info


@pytest.mark.parametrize("heur", list(G.HEURISTICS), ids=list(G.HEURISTICS))
@pytest.mark.parametrize("scene", list(G.SCENES))
def test_one_lane_per_query_answers_every_family_as_the_reading(scene, heur):
    """rayrs_test_intersect (exact = 1)."""
    rays, spans = scene_rays(scene)
    sc, _ = device_scene(scene, heur)
    assert_same(intersect(sc, rays.o, rays.d), reading(scene, heur), "rayrs_test_intersect")


@pytest.mark.parametrize("heur", list(G.HEURISTICS), ids=list(G.HEURISTICS))
@pytest.mark.parametrize("scene", list(G.SCENES))
def test_the_render_route_answers_every_family_as_the_reading(scene, heur):
    """rayrs_test_trace (exact = 1): the pre-test and the traversal kernel's rounds."""
    rays, spans = scene_rays(scene)
    sc, info = device_scene(scene, heur)
    t, obj, answered = trace(sc, rays.o, rays.d)
    assert_same((t, obj), reading(scene, heur), "rayrs_test_trace")
    if info["hot_count"] >= 1:
        assert answered > 0          # the pre-test answered some rays outright: they never reached the traversal kernel
    else:
        assert answered == 0


def test_the_hot_group_scenes_have_one_and_the_layouts_differ():
    got = {s: rayrs_amd.Scene(G.SCENES[s](), G.T0, G.T1, G.HEURISTICS["sah1000"], HDRI, device=-1).info()
           for s in ("mesh1280_light", "mesh5120", "soup", "grid_soup", "degenerate", "floor_spheres")}
    assert got["mesh1280_light"]["compact"] == 1 and got["mesh5120"]["compact"] == 1
    assert got["soup"]["compact"] == 0 and got["grid_soup"]["compact"] == 0 and got["floor_spheres"]["compact"] == 0
    assert sum(got[s]["hot_count"] >= 1 for s in got) >= 2
    assert all(got[s]["local_pool"] == 0 for s in HOT_SCENES)


@pytest.mark.parametrize("how", [dict(lab=dict(hot_group=0xffffffff))] + [dict(lab=x) for x in LEAF_QUEUE] +
                         [dict(tuning=dict(pool_slots=1024))],
                         ids=["whole_gate_tree", "queues_fill", "queues_fill_stack_in_hbm", "leaf_phase_at_once",
                              "one_lane_waits", "pool_1024"])
@pytest.mark.parametrize("scene", HOT_SCENES)
def test_the_render_route_answers_as_the_reading_however_it_is_set(scene, how):
    """rayrs_test_trace on the hot-group scenes with other rayrs_lab / rayrs_tuning settings."""
    rays, spans = scene_rays(scene)
    want = reading(scene, "sah1000")
    sc = rayrs_amd.Scene(G.SCENES[scene](), G.T0, G.T1, G.HEURISTICS["sah1000"], HDRI, device=0)
    assert sc.info()["hot_count"] >= 1
    sc.lab_set(**how.get("lab", {}))
    sc.set_tuning(**how.get("tuning", {}))
    o, d = rays.o, rays.d
    if "tuning" in how:   # several thousand rays through 1024 slots: many chunks, each its windows and rounds
        assert len(o) > 32 * 1024
    t, obj, answered = trace(sc, o, d)
    assert_same((t, obj), want, f"rayrs_test_trace {how}")
    if how.get("lab", {}).get("hot_group") == 0xffffffff:
        assert answered == 0      # no hot group: no pre-test
    else:
        assert answered > 0


@pytest.mark.parametrize("hot_records", [0xffffffff, 1], ids=["every_record_from_hbm", "first_record_from_lds"])
@pytest.mark.parametrize("scene", ["mesh1280_light", "soup"])
def test_the_record_test_answers_alike_from_either_source(scene, hot_records):
    """Both walks' interior steps share one record test, which fetches a record from its LDS copy or from HBM, in the compact
    (mesh1280_light: with a hot group) and in the f64 layout (soup).  rayrs_lab hot_records says how many records are
    copied to LDS: none, or the first only, so that one walk reads from both.  The default walk (exact = 1) is held to the
    reading; the fast walk (exact = 0) promises nothing against the reading and is held to itself under default settings."""
    rays, spans = scene_rays(scene)
    sc, info = device_scene(scene, "sah1000")
    # some records of either walk's tree are left in HBM when the first is in LDS
    assert info["n_wide"] > 1 and (info["hot_n_wide"] if info["hot_count"] else info["gate_n_wide"]) > 1
    fast = trace(sc, rays.o, rays.d, exact=0)[:2]
    sc.lab_set(hot_records=hot_records)
    assert_same(trace(sc, rays.o, rays.d)[:2], reading(scene, "sah1000"), f"rayrs_test_trace hot_records={hot_records:#x}")
    assert_same(trace(sc, rays.o, rays.d, exact=0)[:2], fast, f"rayrs_test_trace exact=0 hot_records={hot_records:#x}")
