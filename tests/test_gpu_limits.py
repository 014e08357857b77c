"""The path pool's numbering limits, rendered and compared with the oracle bit for bit.

The launch accepts image sides up to 65535 pixels (TailSlot::pix is row << 16 | col) and frames of up to 2^32 - 1
(pixel, chunk) items (item ids are uint32_t: wavefront.hip next_sample, local_pool.hip lp_gen, layout.h item_geometry).
Frames at those limits: the widest and the tallest image, and item ids past 2^31 on both routes -- on the local pool
spread over about 32 segments of whole tiles (frame_plan.cpp plan_frame), whose last one ends the frame."""
import numpy as np
import pytest
import torch

import _oracle
import rayrs_amd
from rayrs_amd import _ffi, procedural, scenes
from test_gpu_render import assert_same_frame

pytestmark = pytest.mark.gpu

HDRI = procedural.make_hdri(256, 128)
COUNTERS = ("rays", "paths", "escaped_paths", "nan_pixels", "neg_pixels")


def setup(w, h):
    cam_args, objs, heur = scenes.diffuse_single_sphere()
    cam_args = scenes.camera_for_resolution(cam_args, w, h)
    scene = rayrs_amd.Scene(objs, 1e-6, 1e6, heur, HDRI, device=0)
    cam = rayrs_amd.Camera(*cam_args)
    assert (cam.x_pixels(), cam.y_pixels()) == (w, h)
    osc = _oracle.OracleScene(objs, 1e-6, 1e6, heur, HDRI)
    return scene, cam, osc, _oracle.OracleCamera(*cam_args)


@pytest.mark.parametrize("w,h", [(65535, 2), (2, 65535)], ids=["widest", "tallest"])
def test_widest_and_tallest_images(w, h):
    scene, cam, osc, ocam = setup(w, h)
    ref, ost = osc.render(ocam, 1, 50, traversal=0)
    for local_pool in (0, 1):
        scene.set_tuning(local_pool=local_pool)
        img, st = rayrs_amd.render(scene, cam, 1, 50, out_f64=True)
        assert st["local_pool"] == (1 if local_pool == 0 else 0)
        assert_same_frame(img, ref)
        for k in COUNTERS:
            assert st[k] == ost[k], (local_pool, k)
    # three tile shares into one buffer (the last, tile_rank = 2, on its own numbering of the tiles)
    img, tot = None, {}
    for r in range(3):
        img, st = rayrs_amd.render(scene, cam, 1, 50, out_f64=True, tile_rank=r, tile_ranks=3, out=img)
        for k in COUNTERS:
            tot[k] = tot.get(k, 0) + st[k]
    assert_same_frame(img, ref)
    for k in COUNTERS:
        assert tot[k] == ost[k], k


def test_a_side_of_65536_pixels_is_refused():
    cam_args, objs, heur = scenes.diffuse_single_sphere()
    scene = rayrs_amd.Scene(objs, 1e-6, 1e6, heur, HDRI, device=0)
    for w, h in ((65536, 2), (2, 65536)):
        cam = rayrs_amd.Camera(*scenes.camera_for_resolution(cam_args, w, h))
        with pytest.raises(_ffi.RayrsError) as e:
            rayrs_amd.render_launch(scene, cam, rayrs_amd.make_params(1, 4), 16, 0)  # refused before the buffer is touched
        assert e.value.status == -5


def compare_bands(img, st, osc, ocam, spp, bands):
    for r0, r1 in bands:
        ref, ost = osc.render(ocam, spp, 50, sample_chunk=1, rows=(r0, r1), traversal=0)
        assert_same_frame(img[r0:r1], ref[r0:r1])
        assert ost["paths"] == (r1 - r0) * ocam.x_pixels() * spp
    assert st["nan_pixels"] == 0 and st["neg_pixels"] == 0


def test_item_ids_past_2_31_on_the_local_pool():
    """4096 x 4096 at 255 spp, one sample per item: 262,144 tiles x 255 chunks x 64 = 4,278,190,080 items, just below 2^32,
    in 32 segments of 8225 tiles.  Bands: the first rows; the tile row whose items cross 2^31 (tile 131,586 starts at item
    2^31 - 128); rows inside the last segment (from tile row 498); the last rows of the frame."""
    spp = 255
    scene, cam, osc, ocam = setup(4096, 4096)
    assert scene.info()["local_pool"] == 1
    img, st = rayrs_amd.render(scene, cam, spp, 50, sample_chunk=1, out_f64=True)
    assert st["local_pool"] == 1 and st["kernel_launches"] == 32
    assert st["paths"] == 4096 * 4096 * spp
    compare_bands(img, st, osc, ocam, spp, [(0, 2), (2056, 2058), (4000, 4002), (4094, 4096)])


def test_item_ids_past_2_31_on_the_streaming_route():
    """1024 x 1024 at 2100 spp, one sample per item: 2,202,009,600 items through a pool of 2^24 slots.  The streaming
    route keeps every item's sum until the frame is resolved (24 bytes each, 53 GB)."""
    spp = 2100
    items = 1024 * 1024 * spp
    need = items * 24 + (1 << 24) * 161 + (2 << 30)   # item sums, the pool (a slot, its light entry, its state), headroom
    free, _ = torch.cuda.mem_get_info(0)
    if free < need:
        pytest.skip(f"needs {need / 2**30:.1f} GiB of free device memory, {free / 2**30:.1f} GiB free")
    scene, cam, osc, ocam = setup(1024, 1024)
    scene.set_tuning(local_pool=1, pool_slots=1 << 24)
    img, st = rayrs_amd.render(scene, cam, spp, 50, sample_chunk=1, out_f64=True)
    assert st["local_pool"] == 0 and st["paths"] == items
    compare_bands(img, st, osc, ocam, spp, [(0, 2), (1022, 1024)])
