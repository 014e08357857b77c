"""Radiance queries (include/rayrs_hip.h RADIANCE QUERY, IRRADIANCE) without a GPU: the entry points are declared and exported,
every refusal that is decided before the device is touched comes in the header's order, the wrapper checks its inputs first, the
kernels keep their resources, and the plain-Python reading (tests/_radiance.py) sums as the header says."""
import os
import re

import numpy as np
import pytest

import _film
import _radiance
import rayrs_amd
from rayrs_amd import _ffi
from test_features import HIPCC, compile_asm, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["rayrs_scene_radiance", "rayrs_scene_radiance_launch", "rayrs_scene_irradiance", "rayrs_scene_irradiance_launch"]
LAB_SYMBOLS = ["rayrs_lab_radiance_tuning", "rayrs_lab_radiance_turns"]
INVALID_ARG, NO_DEVICE, UNSUPPORTED = -1, -4, -5


def header():
    return open(os.path.join(ROOT, "include", "rayrs_hip.h")).read()


def test_the_header_declares_the_entry_points_with_their_contract():
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\bint {name}\s*\(", code), name
    text = re.sub(r"\s+", " ", re.sub(r"\s*\n \*\s*", " ", header()))
    assert "RADIANCE QUERY, specified to the operation" in text
    assert "key = rr_path_key(seed, index_base + i, s); rng = (key, draw 0)" in text
    assert "L_{i,s} = radiance(scene, Ray{o_i, d_i}, max_bounces)" in text
    assert "C_k = Vec3::zeros(); C_k += L_{i,s} in sample order" in text
    assert "sum_i = C_0 assigned, then += C_k in chunk order" in text
    assert "radiance_i = sum_i * (1.0 / (double)S)" in text
    assert "queries_i = the number of Bvh::intersect calls of the ray's S paths (u32)" in text
    assert "with the path's rng continuing at draw 2" in text
    assert "the cosine-weighted mean of the incoming radiance, E / pi" in text
    assert text.index("AMBIENT OCCLUSION, specified") < text.index("RADIANCE QUERY, specified") < text.index("IRRADIANCE. A point")
    assert int(re.search(r"#define RAYRS_ABI_VERSION (\d+)", header()).group(1)) == 7
    lab = open(os.path.join(ROOT, "rayrs_amd", "csrc", "rayrs_lab.h")).read()
    for name in LAB_SYMBOLS:
        assert re.search(rf"\bint {name}\s*\(", lab), name
    assert "shade_at" not in re.search(r"typedef struct \{(.*?)\} rayrs_lab_tuning;", lab, re.S).group(1)


def test_the_binding_declares_and_the_library_exports_the_entry_points():
    L = _ffi.lib()
    assert L.rayrs_abi_version() == _ffi.ABI_VERSION == 7
    for name in NEW_SYMBOLS:
        assert name in _ffi.SYMBOLS and hasattr(L, name) and getattr(L, name).argtypes, name
    for name in LAB_SYMBOLS:
        assert name in _ffi.PRIVATE_SYMBOLS and hasattr(L, name) and getattr(L, name).argtypes, name
    assert hasattr(rayrs_amd.Scene, "radiance") and hasattr(rayrs_amd.Scene, "irradiance")
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"fn {name}\(", text), name


def host_scene():
    cam_args, objs, heur, env = _film.sphere_desc()
    return rayrs_amd.Scene(objs, 1e-6, 1e6, heur, env, device=-1)


@pytest.mark.parametrize("n", [4, 0])
def test_refusals_on_a_host_only_scene_come_in_the_headers_order(n):
    """RAYRS_INVALID_ARG (a NULL scene or input, both outputs NULL, samples == 0, fast_traversal > 1) whatever else is wrong
    beside it, then RAYRS_UNSUPPORTED (the sizes), and only then RAYRS_NO_DEVICE; one NULL output is accepted up to there."""
    L = _ffi.lib()
    scene = host_scene()
    a, b = np.zeros((4, 3)), np.ones((4, 3))
    rad, cnt = np.zeros((4, 3)), np.zeros(4, dtype=np.uint32)
    P = lambda x: x.ctypes.data

    def call(irr, launch, scene_h=scene._h, a_=P(a), b_=P(b), samples=4, bounces=50, chunk=0, fast=0, rad_=P(rad), cnt_=P(cnt)):
        args = (scene_h, a_, b_, n, samples, bounces, chunk) + ((1e-4,) if irr else ()) + (1, 0, fast, rad_, cnt_)
        name = "rayrs_scene_irradiance" if irr else "rayrs_scene_radiance"
        return getattr(L, name + "_launch")(*args, None) if launch else getattr(L, name)(*args)

    too_big = (dict(samples=1 << 30), dict(bounces=8001), dict(samples=1 << 20, bounces=4096), dict(samples=(1 << 21) + 1, chunk=1, bounces=1),
               dict(samples=(1 << 21) + 2, chunk=2, bounces=1))
    for irr in (False, True):
        for launch in (False, True):
            for bad in (dict(scene_h=None), dict(a_=None), dict(b_=None), dict(rad_=None, cnt_=None), dict(samples=0), dict(fast=2),
                        dict(fast=0xffffffff)):
                assert call(irr, launch, **bad) == INVALID_ARG, (irr, launch, bad)
                if "samples" not in bad:
                    assert call(irr, launch, bounces=8001, **bad) == INVALID_ARG
                    assert call(irr, launch, samples=1 << 30, **bad) == INVALID_ARG
            for big in too_big:
                assert call(irr, launch, **big) == UNSUPPORTED, (irr, launch, big)
            # the limits themselves, and a ray of exactly 2^20 chunks, pass up to the device
            for ok in (dict(), dict(fast=1), dict(rad_=None), dict(cnt_=None), dict(bounces=0), dict(bounces=8000), dict(samples=(1 << 30) - 1, bounces=4),
                       dict(samples=1 << 20, chunk=1, bounces=4095)):
                assert call(irr, launch, **ok) == NO_DEVICE, (irr, launch, ok)
    if n:
        for f in (scene.radiance, scene.irradiance):
            with pytest.raises(_ffi.RayrsError) as e:
                f(a, b)
            assert e.value.status == NO_DEVICE
    assert L.rayrs_lab_radiance_tuning(None, 1, 1, 1) == INVALID_ARG
    for bad in ((65, 1, 1), (1, 65, 1), (1, 1, 65)):
        assert L.rayrs_lab_radiance_tuning(scene._h, *bad) == INVALID_ARG
    assert L.rayrs_lab_radiance_tuning(scene._h, 64, 64, 64) == 0 and L.rayrs_lab_radiance_tuning(scene._h, 0, 0, 0) == 0


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the wrapper called {name} before it checked its inputs")


def test_the_wrapper_refuses_bad_shapes_before_any_library_call(monkeypatch):
    scene = host_scene()
    monkeypatch.setattr(scene, "_L", NoLibrary())
    good = np.zeros((5, 3))
    for f, name in ((scene.radiance, "rayrs_scene_radiance"), (scene.irradiance, "rayrs_scene_irradiance")):
        for bad_a, bad_b in ((np.zeros((5, 2)), good), (good, np.zeros((4, 3))), (np.zeros(15), np.zeros(15))):
            with pytest.raises(ValueError):
                f(bad_a, bad_b)
        for samples in (0, -1):
            with pytest.raises(ValueError):
                f(good, good, samples=samples)
        with pytest.raises(AssertionError, match=name):
            f(good, good)


# ---- kernel resources.  kernels.hip's test_path_trace_kernel, the radiance loop fused with the walk in one lane, takes 157 / 159
# registers: the three-wave class (512 // 3 = 170, allocated in eights: 168).  radiance_kernel carries a lane's whole state across
# its turns on top of that and is held to the two-wave class, 256, and to no scratch at all.
VGPR_BOUND = 256


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_the_radiance_kernels_use_no_scratch_and_keep_two_waves_per_simd(tmp_path):
    res = kernel_resources(compile_asm("radiance.hip", tmp_path))
    path = {n: r for n, r in res.items() if "radiance_kernel" in n}
    resolve = {n: r for n, r in res.items() if "radiance_resolve_kernel" in n}
    assert len(path) == 16 and len(resolve) == 1 and len(res) == 17   # COMPACT x EXACT x IRRADIANCE x STEPS; the resolve
    for name, (vgpr, scratch, lds) in res.items():
        assert vgpr <= VGPR_BOUND and scratch == 0 and lds == 0, (name, vgpr, scratch, lds)   # (the stacks are dynamic LDS)


def test_the_readings_sum_rule():
    """S = 5 with c = 2 gives chunks of 2, 2 and 1 samples; c = 0 and c >= S one chunk.  The values are chosen so that the order
    of the additions shows in the bits."""
    assert _radiance.chunks(5, 2) == [(0, 2), (2, 4), (4, 5)]
    assert _radiance.chunks(5, 0) == _radiance.chunks(5, 5) == _radiance.chunks(5, 9) == [(0, 5)]
    assert _radiance.chunks(4, 2) == [(0, 2), (2, 4)] and _radiance.chunks(1, 0) == [(0, 1)]
    v = np.array([[1.0, 0.1, -0.0], [2.0 ** 60, 0.2, -0.0], [-2.0 ** 60, 0.3, -0.0], [1.0, 0.4, -0.0], [1.0, 0.7, -0.0]])
    f = np.float64
    inv = f(1.0) / f(5.0)
    zero = f(0.0)
    for k in range(3):
        x = [f(a) for a in v[:, k]]
        chunked = (((zero + x[0]) + x[1]) + ((zero + x[2]) + x[3])) + ((zero + x[4]))
        straight = ((((zero + x[0]) + x[1]) + x[2]) + x[3]) + x[4]
        assert _radiance.mean(v, 2)[k].tobytes() == (chunked * inv).tobytes()
        assert _radiance.mean(v, 0)[k].tobytes() == _radiance.mean(v, 7)[k].tobytes() == (straight * inv).tobytes()
    assert _radiance.mean(v, 2)[0] != _radiance.mean(v, 0)[0]
    assert np.signbit(v[:, 2]).all() and not np.signbit(_radiance.mean(v, 0)[2])   # (zeros() + -0 is +0)
    rad, q = _radiance.answers(v[None], np.array([[1, 2, 3, 4, 5]]), 2)
    assert rad.shape == (1, 3) and q.dtype == np.uint32 and q.tolist() == [15]
