"""The item hand-out (wavefront.hip next_sample, local_pool.hip lp_gen) where a wave's last reserved range is cut short.

The small frames of the other GPU tests have a tile count that is a multiple of 4, so their item counts are multiples of
the streaming route's reserve of 256 and no range ever ends before its reserve does.  Here the frame is 21 x 7 pixels:
three 8x8 tiles with one padding row and three padding columns, 5 samples in chunks of 1 -- 960 items, 3.75 reserves of
256, 735 paths (padding pixels start none).  Every frame is the oracle's bit for bit, and so are the counters."""
import functools

import numpy as np
import pytest

import _oracle
import rayrs_amd
from rayrs_amd import procedural, scenes

pytestmark = pytest.mark.gpu

W, H, SPP, CHUNK, SEED = 21, 7, 5, 1, 0x5EED
PATHS = W * H * SPP
HDRI = procedural.make_hdri(256, 128)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


@functools.lru_cache(maxsize=None)
def setup(name):
    cam_args, objs, heur = scenes.material_test() if name == "material_test" else scenes.mesh_scene(4)
    cam_args = scenes.camera_for_resolution(cam_args, W, H)
    scene = rayrs_amd.Scene(objs, 1e-6, 1e6, heur, HDRI, device=0)
    osc = _oracle.OracleScene(objs, 1e-6, 1e6, heur, HDRI)
    return scene, rayrs_amd.Camera(*cam_args), osc, _oracle.OracleCamera(*cam_args)


@functools.lru_cache(maxsize=None)
def oracle(name, max_bounces):
    _, _, osc, ocam = setup(name)
    return osc.render(ocam, SPP, max_bounces, seed=SEED, sample_chunk=CHUNK, traversal=0)


def render(scene, cam, max_bounces):
    return rayrs_amd.render(scene, cam, SPP, max_bounces, seed=SEED, sample_chunk=CHUNK, out_f64=True)


def check(name, max_bounces, img, st):
    ref, ost = oracle(name, max_bounces)
    assert not np.isnan(ref).any()
    print(name, max_bounces, {k: (st[k], ost[k]) for k in ("paths", "rays", "escaped_paths")})
    assert np.array_equal(bits(img), bits(ref))
    for k in ("paths", "rays", "escaped_paths"):
        assert st[k] == ost[k], k
    assert st["paths"] == PATHS


@pytest.fixture
def material_scene():
    scene, cam, _, _ = setup("material_test")
    yield scene, cam
    scene.set_tuning()
    scene.lab_set()


def test_the_streaming_route_cuts_its_fourth_reserve_at_960_items(material_scene):
    """192 slots, five items each; the fourth reserve of 256 ends at 960, every wave then finds the counter exhausted
    and remembers it across the round's launches."""
    scene, cam = material_scene
    scene.set_tuning(local_pool=1, pool_slots=192)
    img, st = render(scene, cam, 50)
    assert st["kernel_launches"] > 1
    check("material_test", 50, img, st)


@pytest.mark.parametrize("reserve", [9, 4096])
def test_the_local_pool_with_a_reserve_that_does_not_divide_the_items_and_one_that_covers_them(material_scene, reserve):
    """9: 960 is no multiple of it, and a batch of 64 lanes needs many turns of the hand-out loop.  4096: the first wave's
    reserve covers the segment and every other wave finds nothing."""
    scene, cam = material_scene
    scene.lab_set(local_reserve=reserve)
    img, st = render(scene, cam, 50)
    assert st["kernel_launches"] == 1
    check("material_test", 50, img, st)


@pytest.mark.parametrize("route", ["streaming", "local"])
def test_no_bounces_answers_every_item_in_the_hand_out(material_scene, route):
    """radiance() with an empty loop: every item's sum is zeros, written where the item is handed out; only real pixels'
    samples count as paths."""
    scene, cam = material_scene
    if route == "streaming":
        scene.set_tuning(local_pool=1, pool_slots=192)
    img, st = render(scene, cam, 0)
    assert (st["kernel_launches"] == 1) == (route == "local")
    assert not bits(img).any()
    assert st["paths"] == 735 and st["rays"] == 0
    check("material_test", 0, img, st)


def test_a_hot_group_scene_on_a_pool_of_two_windows():
    """The pre-tested READY lists and the batch carry between windows, with the cut-short reserve."""
    scene, cam, _, _ = setup("mesh_scene")
    assert scene.info()["hot_count"] >= 1
    scene.set_tuning(local_pool=1, pool_slots=192)
    try:
        img, st = render(scene, cam, 50)
    finally:
        scene.set_tuning()
    assert st["hot_group"] == 1
    check("mesh_scene", 50, img, st)
