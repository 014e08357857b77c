"""Paths that run to the bounce budget, compared with the oracle bit for bit.

In the reference's scenes every path ends within tens of bounces (albedo <= 0.8, then Russian roulette), so the pool's
narrow per-path fields -- bounce and RNG draw index packed as `bounce | draw << 16` (wavefront.h RaySlot::bd; 15 + 16 bits
in the local pool) -- never get near the 8000-bounce budget the launch accepts, and a frame's long tail (a handful of slots
live for thousands of rounds: 4-round batches, the traversal kernel's static windows once few slots are live, a leaf queue
with one waiting lane, rounds beyond the MAX_TIMED events of render.cpp) is never rendered.  Here the rooms are closed and
their surfaces scatter with a weight of exactly (1, 1, 1), so `rng_next() > max(throughput) = 1` never fires
(lib.rs:539-545) and every path runs to its budget; or their weights are close to one and some paths run to 8000 bounces
drawing four numbers at each, the case the limit is derived from (draw index 2 + 4 x 8000 = 32002)."""
import ctypes as C

import numpy as np
import pytest

import _oracle
import rayrs_amd
from rayrs_amd import _ffi, procedural, scenes
from rayrs_amd.api import Axis, BvhHeuristic, Emission, Material, Object
from test_gpu_render import assert_same_frame

pytestmark = pytest.mark.gpu

HDRI = procedural.make_hdri(256, 128)
WHITE = (1.0, 1.0, 1.0)
DARK = Emission.Dark()
LIGHT = Emission.new(0.5, (1.0, 0.9, 0.8))
ROOM_CAM = ((0.0, 0.0, 2.5), (0.0, 1.0, 0.0), (0.0, -0.3, -3.0), 70.0, 4.0, 3.0, 4)
COUNTERS = ("rays", "paths", "escaped_paths", "nan_pixels", "neg_pixels")
# The rooms' near plane.  At the usual 1e-6 a path that bounces within 1e-6 of an edge of the room skips the adjacent wall
# and leaves the room: about one path in a thousand at 8000 bounces.  The kernels take z_near from the scene.
Z_NEAR = 1e-9


def room(wall_mats, inner):
    """A closed 4 x 4 x 6 box of six planes whose normals face inward (Object.box_geom's do not all: lib.rs:438-506),
    the ceiling emissive, the camera inside.  Each wall reaches half a unit past the others, so that no ray leaves
    through a seam where two walls meet."""
    a, b = 2.5, 3.5
    walls = [Object.plane(Axis.X, -a, a, -b, b, -2., wall_mats[0], DARK),
             Object.plane(Axis.XRev, -a, a, -b, b, 2., wall_mats[1], DARK),
             Object.plane(Axis.Y, -a, a, -b, b, -2., wall_mats[2], DARK),
             Object.plane(Axis.YRev, -a, a, -b, b, 2., wall_mats[3], LIGHT),
             Object.plane(Axis.Z, -a, a, -a, a, -3., wall_mats[4], DARK),
             Object.plane(Axis.ZRev, -a, a, -a, a, 3., wall_mats[5], DARK)]
    return ROOM_CAM, walls + inner, BvhHeuristic.Sah(1000)


def white_room():
    """Lambertian, mirror and glass surfaces of colour (1, 1, 1): the weight of every scattering event is exactly one."""
    lam, mirror = Material.LambertianDiffuse(WHITE), Material.Reflect(WHITE)
    return room([lam, mirror, lam, lam, lam, lam],
                [Object.sphere(0.8, (0.8, -0.9, -0.6), Material.Glass(WHITE, 1.5), DARK),
                 Object.sphere(0.6, (-1.0, -1.1, 0.5), mirror, DARK)])


def plastic_room():
    """Plastic walls (a Fresnel draw, then a Lambertian or a Cook-Torrance lobe: four draws per bounce with the roulette's)
    and a Cook-Torrance glass sphere (four as well).  The Lambertian lobe's weight is exactly one; the glossy lobes' are
    not, so most paths end after some hundreds of bounces and a few run to 8000 (index of refraction 1 keeps the
    glossy lobe rare, a small roughness keeps its weight near one)."""
    pl = Material.Plastic(WHITE, WHITE, 0.005, 1.0)
    return room([pl] * 6, [Object.sphere(0.3, (0.8, -0.9, -0.6), Material.CookTorranceGlass(WHITE, 0.01, 1.5), DARK)])


def hot_room():
    """scenes.mesh_scene(3)'s floor and 1280-triangle mesh, all white, with five walls around them (one a mirror, the
    ceiling emissive): a scene of the streaming route whose floor is the hot group (wavefront.hip finish_rays)."""
    _, objs, heur = scenes.mesh_scene(3, mat=Material.LambertianDiffuse(WHITE))
    lam = Material.LambertianDiffuse(WHITE)
    objs[0].mat = lam
    objs += [Object.plane(Axis.X, 0., 5., -3., 4., -3., lam, DARK), Object.plane(Axis.XRev, 0., 5., -3., 4., 3., lam, DARK),
             Object.plane(Axis.YRev, -3., 3., -3., 4., 5., lam, LIGHT),
             Object.plane(Axis.Z, -3., 3., 0., 5., -3., lam, DARK),
             Object.plane(Axis.ZRev, -3., 3., 0., 5., 4., Material.Reflect(WHITE), DARK)]
    return scenes.MESH_CLOSE_CAM, objs, heur


def setup(scene_fn, w, h):
    cam_args, objs, heur = scene_fn()
    cam_args = scenes.camera_for_resolution(cam_args, w, h)
    scene = rayrs_amd.Scene(objs, Z_NEAR, 1e6, heur, HDRI, device=0)
    osc = _oracle.OracleScene(objs, Z_NEAR, 1e6, heur, HDRI)
    return scene, rayrs_amd.Camera(*cam_args), osc, _oracle.OracleCamera(*cam_args)


def assert_same(img, st, ref, ost):
    assert_same_frame(img, ref)
    for k in COUNTERS:
        assert st[k] == ost[k], k


@pytest.mark.parametrize("budget", [1500, 8000])
def test_white_room_every_path_runs_to_its_budget(budget):
    """Both routes (the local pool, the scene's own; streaming through the pool in HBM) and both walks."""
    w, h, spp = 24, 16, 2
    scene, cam, osc, ocam = setup(white_room, w, h)
    assert scene.info()["local_pool"] == 1
    ref, ost = osc.render(ocam, spp, budget, traversal=0)
    assert ost["rays"] == ost["paths"] * budget == w * h * spp * budget and ost["escaped_paths"] == 0
    for local_pool in (0, 1):
        scene.set_tuning(local_pool=local_pool)
        for fast in (False, True):
            img, st = rayrs_amd.render(scene, cam, spp, budget, out_f64=True, fast_traversal=fast)
            assert st["local_pool"] == (1 if local_pool == 0 else 0)
            assert_same(img, st, ref, ost)


def test_plastic_room_at_the_bounce_limit():
    """The frame at budget 8000 on both routes, and one path that reaches bounce 8000 with a draw index >= 30000, bounce
    by bounce (rayrs_test_path_trace).  The trace hook runs a sample's loop in one thread with the bounce and draw index
    in registers: it does not go through the pool's packed `bounce | draw << 16` words, which only the frame comparison
    covers."""
    budget, w, h, spp = 8000, 32, 24, 2
    scene, cam, osc, ocam = setup(plastic_room, w, h)
    ref, ost = osc.render(ocam, spp, budget, traversal=0)
    for local_pool in (0, 1):
        scene.set_tuning(local_pool=local_pool)
        img, st = rayrs_amd.render(scene, cam, spp, budget, out_f64=True)
        assert_same(img, st, ref, ost)
    # the frame's samples on the oracle, counted, then the first two that reach bounce 8000 traced in full
    pix = np.array([(r, c) for r in range(h) for c in range(w) for _ in range(spp)], dtype=np.uint32)
    sam = np.array([s for _ in range(h * w) for s in range(spp)], dtype=np.uint32)
    n_all = osc.path_traces(ocam, [tuple(p) for p in pix], sam, 0x5EED, budget, cap=1)["n"]
    cand = np.flatnonzero(n_all == budget)[:2]
    assert len(cand) > 0, "no sample of the frame runs to the budget"
    cap = budget
    tr = osc.path_traces(ocam, [tuple(p) for p in pix[cand]], sam[cand], 0x5EED, budget, cap=cap)
    assert (tr["draw"][:, budget - 1] >= 30000).all()
    k = cand
    packed = np.ascontiguousarray((pix[k, 0] << 16) | pix[k, 1], dtype=np.uint32)
    ks = np.ascontiguousarray(sam[k])
    n = np.zeros(len(k), dtype=np.uint32); obj = np.zeros((len(k), cap), dtype=np.int64); t = np.zeros((len(k), cap))
    thr = np.zeros((len(k), cap, 3)); draw = np.zeros((len(k), cap), dtype=np.uint32); rgb = np.zeros((len(k), 3))
    _ffi.check(scene._L.rayrs_test_path_trace(scene._h, C.byref(cam.desc), 0x5EED, budget, packed.ctypes.data,
                                              ks.ctypes.data, len(k), 1, cap, n.ctypes.data, obj.ctypes.data,
                                              t.ctypes.data, thr.ctypes.data, draw.ctypes.data, rgb.ctypes.data),
               "rayrs_test_path_trace")
    assert np.array_equal(n, tr["n"]) and np.array_equal(obj, tr["obj"]) and np.array_equal(draw, tr["draw"])
    for got, want in ((t, tr["t"]), (thr, tr["thr"]), (rgb, tr["rgb"])):
        assert np.array_equal(got.view(np.uint64), np.ascontiguousarray(want).view(np.uint64))


@pytest.mark.parametrize("lab", [dict(), dict(leaf_min=64, leaf_wait=1, refill_min=1)], ids=["default", "one_lane_waits"])
def test_hot_group_room_streams_every_path_to_its_budget(lab):
    """Thousands of rounds through finish_rays' pre-test and the default walk's leaf queues, with the lab's default
    thresholds and with test_gpu_hot_group.py's most extreme ones (a leaf phase waits for all 64 lanes, or one)."""
    budget, w, h, spp = 8000, 16, 12, 2
    scene, cam, osc, ocam = setup(hot_room, w, h)
    info = scene.info()
    assert info["local_pool"] == 0 and info["hot_count"] > 0
    ref, ost = osc.render(ocam, spp, budget, traversal=0)
    assert ost["rays"] == w * h * spp * budget
    scene.lab_set(**lab)
    img, st = rayrs_amd.render(scene, cam, spp, budget, out_f64=True)
    assert st["hot_group"] == 1
    assert_same(img, st, ref, ost)


def test_more_rounds_than_timed_rounds():
    """A pool of 1024 slots for 2048 paths of 8000 bounces each: slots take two samples one after the other and the
    frame runs about 16000 rounds, past the 8192 rounds whose kernel times are recorded (render.cpp MAX_TIMED).  The frame
    and counters are the oracle's, the round times stop at 8192 without an error, and an ordinary frame rendered next on
    the same scene is the oracle's too (counters, wave_items and the item counter are reset after a long frame)."""
    budget, w, h, spp = 8000, 32, 16, 4
    scene, cam, osc, ocam = setup(white_room, w, h)
    scene.set_tuning(local_pool=1, pool_slots=1024)
    ref, ost = osc.render(ocam, spp, budget, sample_chunk=1, traversal=0)
    img, st = rayrs_amd.render(scene, cam, spp, budget, sample_chunk=1, out_f64=True)
    assert st["local_pool"] == 0 and st["kernel_launches"] > 8192   # (the streaming route counts its rounds here)
    assert_same(img, st, ref, ost)
    L = scene._L
    L.rayrs_lab_round_ms.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    L.rayrs_lab_round_ms.restype = C.c_int
    n_timed = L.rayrs_lab_round_ms(scene._h, None, 0)
    assert n_timed == 8192
    ms = np.zeros((n_timed, 3), dtype=np.float32)
    assert L.rayrs_lab_round_ms(scene._h, ms.ctypes.data, n_timed) == 8192
    assert np.isfinite(ms).all() and (ms >= 0).all()
    # an ordinary frame behind it
    ref2, ost2 = osc.render(ocam, 3, 50, seed=17, traversal=0)
    img2, st2 = rayrs_amd.render(scene, cam, 3, 50, seed=17, out_f64=True)
    assert_same(img2, st2, ref2, ost2)
