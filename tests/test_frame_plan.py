"""A frame's plan (rayrs_amd/csrc/frame_plan.cpp plan_frame) without a GPU and without a scene: the arithmetic that decides
a render's items, segments, pool, grids and buffer sizes, held to figures derived elsewhere in the project (the
docstrings of test_gpu_limits.py and test_gpu_film_sizes.py, bench.py's memory forecast) and to its own invariants on random
requests.  tests/frame_plan_probe.cpp links frame_plan.cpp alone -- no HIP runtime -- under the address and
undefined-behaviour sanitizers (linked statically: the program runs whatever else is preloaded)."""
import os
import random
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "rayrs_amd", "csrc")
UNSUPPORTED = -5   # include/rayrs_hip.h RAYRS_UNSUPPORTED
# an MI355X and the kernels as they are built: 256 CUs, windows of 512 slots, five traversal and three local-pool workgroups per CU
DEVICE = dict(cus=256, window=512, bpc=5, local_bpc=3, depth=20, lds=8)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("frame_plan") / "frame_plan_probe"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", str(exe),
                    os.path.join(HERE, "frame_plan_probe.cpp"), os.path.join(CSRC, "frame_plan.cpp")],
                   check=True, capture_output=True)

    def plan(*cases):
        text = "".join(" ".join(f"{k}={v}" for k, v in {**DEVICE, "ranks": 1, **c}.items()) + "\n" for c in cases)
        out = subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True)
        assert out.stderr == ""
        plans = [{k: int(v) for k, v in (w.split("=") for w in line.split())} for line in out.stdout.splitlines()]
        assert len(plans) == len(cases)
        return plans
    return plan


def test_the_headline_frame(probe):
    """2048 x 2048, 1024 spp in chunks of 4 on the streaming route: 2^30 items of 24 bytes, the pool at its cap of 2^28 slots
    (524,288 windows), the shading kernels' grid at 24 workgroups per CU, half of the windows dealt round robin in whole
    rounds of the traversal grid's 5120 waves."""
    p, = probe(dict(w=2048, h=2048, spp=1024, chunk=4))
    assert p["status"] == 0 and p["use_local"] == 0 and p["exact"] == 1
    assert p["total_items"] == 1 << 30 and p["nchunks"] == 256 and p["n_local_tiles"] == 65536
    assert p["live_total"] == p["np"] == 1 << 28
    assert p["np"] // 512 == 524288
    assert p["flat_blocks"] == 6144 == 256 * 24
    assert p["trav_blocks"] == 1280
    assert p["static_windows"] == 261120 == 262144 // 5120 * 5120
    assert p["partial_bytes"] == (1 << 30) * 24
    assert p["pool_bytes"] == (1 << 28) * 161   # a 128-byte slot, a 32-byte light entry, a state byte
    assert p["spill_words"] == (20 - 8) * 1280 * 256 and p["spill_bytes"] == 4 * p["spill_words"]
    assert p["wave_items_bytes"] == 6144 * 4 * 16
    assert p["local_blocks"] == 0 and p["local_light_bytes"] == 0
    assert (p["refill_min"], p["leaf_min"], p["leaf_wait"]) == (52, 48, 16)


def test_the_headline_frame_as_one_rank_of_eight(probe):
    """DESIGN's "44.7 M": one slot per 12 samples of the share's 8192 tiles, in whole windows."""
    p, = probe(dict(w=2048, h=2048, spp=1024, chunk=4, rank=0, ranks=8))
    assert p["n_local_tiles"] == 8192 and p["total_items"] == 1 << 27
    assert p["live_total"] == 44739242 == 8192 * 64 * 1024 // 12
    assert p["np"] == 44739584


def test_a_local_pool_frame_past_2_31_items(probe):
    """test_gpu_limits.py's frame: 4096 x 4096, 255 spp in chunks of 1 on the local-pool route."""
    p, = probe(dict(w=4096, h=4096, spp=255, chunk=1, local_ok=1))
    assert p["status"] == 0 and p["use_local"] == 1
    assert p["total_items"] == 4278190080
    assert p["seg_tiles"] == 8225 and p["seg_items"] == 134232000 == 8225 * 255 * 64
    assert -(-p["total_items"] // p["seg_items"]) == 32
    assert p["partial_need"] == 134232000 and p["partial_bytes"] == 134232000 * 24
    assert p["local_blocks"] == 768
    assert p["np"] == 0 and p["flat_blocks"] == 0 and p["pool_bytes"] == 0 and p["spill_bytes"] == 0


def test_refusals(probe):
    """2^32 items and more; and, on the local-pool route only, a segment of 2^32 items and more.  Segments are whole tiles:
    one tile of 2^31 + 64 items (8 x 8 pixels, 2^25 + 1 chunks) under the lab's largest segment size, 2^32 - 1, makes
    segments of two tiles.  (With the default segment size one tile's chunks reach 2^32 only where the frame's items do.)"""
    lab = {"lab.local_segment_items": 0xffffffff}
    big, seg_local, seg_stream = probe(dict(w=8192, h=8192, spp=4096, chunk=8),
                                       dict(w=8, h=8, spp=(1 << 25) + 1, chunk=1, local_ok=1, **lab),
                                       dict(w=8, h=8, spp=(1 << 25) + 1, chunk=1, local_ok=0, **lab))
    assert big["status"] == UNSUPPORTED and big["total_items"] == 1 << 35
    assert seg_local["total_items"] == (1 << 31) + 64 and seg_local["seg_items"] == (1 << 32) + 128
    assert seg_local["use_local"] == 1 and seg_local["status"] == UNSUPPORTED
    assert seg_stream["total_items"] == (1 << 31) + 64 and seg_stream["use_local"] == 0 and seg_stream["status"] == 0


def test_edges(probe):
    tiny, listed, many, clamped = probe(
        dict(w=8, h=8, spp=1, local_ok=1),                                    # 64 items: fewer than a wave's 112 resident paths
        dict(w=512, h=512, spp=8, chunk=4, has_list=1, n_list=37),            # a film pass over 37 of the share's 4096 tiles
        dict(w=2048, h=2048, spp=256, chunk=1, local_ok=1, **{"lab.local_segment_items": 65536}),
        dict(w=64, h=64, spp=4, pool_slots=1 << 30))
    assert tiny["use_local"] == 1 and tiny["total_items"] == 64 and tiny["local_blocks"] == 1
    assert tiny["local_light_bytes"] == 1 * 4 * 112 * 32
    assert listed["n_local_tiles"] == 37 and listed["total_items"] == 37 * 2 * 64
    assert listed["live_total"] == 4736 and listed["np"] == 5120 and listed["flat_blocks"] == 3  # ten windows, four waves a workgroup
    # 2^30 items in segments of 65536 would be 16384 launches: 64 segments of 2^24 items (1024 tiles) instead
    assert many["total_items"] == 1 << 30 and many["seg_items"] == 1 << 24 and many["seg_tiles"] == 1024
    assert -(-many["total_items"] // many["seg_items"]) == 64
    assert clamped["total_items"] == 4096 and clamped["live_total"] == 4096 and clamped["np"] == 4096


def test_invariants_on_random_requests(probe):
    rnd = random.Random(20250)
    cases = []
    for _ in range(400):
        spp = rnd.choice([1, 2, 7, 64, 255, 1024, rnd.randrange(1, 1 << 16)])
        c = dict(w=rnd.randrange(1, 5000), h=rnd.randrange(1, 5000), spp=spp, chunk=rnd.choice([0, 1, 4, rnd.randrange(1, spp + 1)]),
                 cus=rnd.choice([256, rnd.randrange(1, 305)]), bpc=rnd.randrange(1, 9), local_bpc=rnd.randrange(1, 4),
                 window=rnd.choice([256, 512, 1024]), local_ok=rnd.randrange(2), no_local=rnd.randrange(2), fast=rnd.randrange(2),
                 far=rnd.randrange(2), has_hot=rnd.randrange(2), emitter=rnd.randrange(2))
        c["ranks"] = rnd.choice([1, 1, 2, 8, rnd.randrange(1, 65)])
        c["rank"] = rnd.randrange(c["ranks"])
        if rnd.randrange(3) == 0:
            c["pool_slots"] = rnd.randrange(1, 1 << 29)
        if rnd.randrange(4) == 0:
            c.update(has_list=1, n_list=rnd.randrange(0, 1 << 18))
        if rnd.randrange(3) == 0:
            c["lab.local_segment_items"] = rnd.randrange(65536, 1 << 28)
        if rnd.randrange(4) == 0:
            c["lab.flat_blocks_per_cu"] = rnd.randrange(1, 65)
        if rnd.randrange(4) == 0:
            c["lab.static_pct"] = rnd.randrange(1, 101)
        cases.append(c)
    planned = 0
    for c, p in zip(cases, probe(*cases)):
        tiles = -(-c["w"] // 8) * -(-c["h"] // 8)
        share = (tiles - c["rank"] + c["ranks"] - 1) // c["ranks"] if tiles > c["rank"] else 0
        if c.get("has_list"):
            share = min(share, c["n_list"])
        assert p["n_local_tiles"] == share and p["total_items"] == share * p["nchunks"] * 64, c
        assert (p["status"] == UNSUPPORTED) == (p["total_items"] >= 1 << 32), c   # (no segment of these reaches 2^32)
        if p["status"] != 0:
            continue
        planned += 1
        assert p["use_local"] == (c["local_ok"] and not c["no_local"]), c
        assert p["exact"] == (not c["fast"] or c["far"]), c
        assert p["eager_light"] == c["emitter"], c
        assert p["tile_items"] == p["nchunks"] * 64 and p["seg_items"] % p["tile_items"] == 0 and p["seg_items"] > 0, c
        n_seg = -(-p["total_items"] // p["seg_items"])
        assert n_seg <= 64 and n_seg * p["seg_items"] >= p["total_items"], c
        assert p["live_total"] <= p["total_items"], c
        if p["use_local"] or p["total_items"] == 0:
            assert p["np"] == 0 and p["flat_blocks"] == 0 and p["spill_words"] == 0, c
            assert p["partial_need"] == min(p["seg_items"], p["total_items"]), c
            assert (p["local_blocks"] >= 1) == (p["use_local"] == 1 and p["total_items"] > 0), c
            assert p["local_blocks"] <= c["cus"] * c["local_bpc"], c
        else:
            assert p["np"] % 1024 == 0 and p["live_total"] <= p["np"] < p["live_total"] + 1024, c
            assert p["partial_need"] == p["total_items"] and p["local_blocks"] == 0, c
            assert 1 <= p["flat_blocks"] <= c["cus"] * c.get("lab.flat_blocks_per_cu", 24), c
            assert p["flat_blocks"] * 4 <= p["np"] // c["window"] + 3, c   # at most one wave per window
            assert p["static_windows"] <= p["np"] // c["window"] and p["static_windows"] % (p["trav_blocks"] * 4) == 0, c
        assert p["trav_blocks"] == c["cus"] * c["bpc"], c
    assert planned > 300
