"""Ambient occlusion (include/rayrs_hip.h AMBIENT OCCLUSION) without a GPU: the plain-Python reading of the operation
(tests/_ao.py) makes the oracle's Lambertian scatter directions bit for bit, the entry points are declared and exported, every
refusal that is decided before the device is touched comes in the header's order, and the kernel keeps its resources."""
import os
import re

import numpy as np
import pytest

import _ao
import _film
import _oracle
import rayrs_amd
from rayrs_amd import _ffi
from rayrs_amd.api import Material
from test_features import HIPCC, compile_asm, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["rayrs_scene_ambient_occlusion", "rayrs_scene_ambient_occlusion_launch", "rayrs_render_ao"]
LAB_SYMBOLS = ["rayrs_lab_ao_refill", "rayrs_lab_ao_turns"]
INVALID_ARG, NO_DEVICE = -1, -4
AXES = [(1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, -1.0)]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def test_the_readings_directions_are_the_oracles_lambertian_scatter_directions():
    """1,200 (normal, key) pairs: the six axis normals 20 times each with different keys, unit normals, and normals that are
    not unit (used as given).  Material::evaluate takes two draws for each."""
    rng = np.random.default_rng(20)
    free = rng.normal(size=(1080, 3))
    free[:700] /= np.linalg.norm(free[:700], axis=1, keepdims=True)
    normals = np.concatenate([np.array(AXES * 20), free])
    keys = [_ao.path_key(int(rng.integers(0, 2 ** 62)), int(rng.integers(0, 2 ** 24)), int(s)) for s in range(len(normals))]
    got = _ao.directions(normals, keys)
    scattered, _, want, draws = _oracle.material_evaluate(Material.LambertianDiffuse((0.5, 0.5, 0.5)), normals, normals, keys)
    assert len(normals) >= 1000 and scattered.all() and (draws == 2).all()
    bad = np.flatnonzero((bits(got) != bits(want)).any(axis=1))
    assert len(bad) == 0, (len(bad), [(normals[i].tolist(), got[i].tolist(), want[i].tolist()) for i in bad[:3]])


def test_the_readings_rng_is_the_oracles():
    for seed, pixel, sample in ((0x5EED, 0, 0), (0xA0, 1234567, 15), (2 ** 64 - 1, 2 ** 40 + 7, 256)):
        key = _ao.path_key(seed, pixel, sample)
        for draw in (0, 1):
            assert _ao.uniform(key, draw) == float(_oracle.rng_bits(seed, pixel, sample, draw) >> 11) * 2.0 ** -53


def header():
    return open(os.path.join(ROOT, "include", "rayrs_hip.h")).read()


def test_the_header_declares_the_entry_points_with_their_contract():
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\bint {name}\s*\(", code), name
    text = re.sub(r"\s*\n \*\s*", " ", header())
    assert "AMBIENT OCCLUSION, specified to the operation" in text
    assert "key = rr_path_key(seed, index_base + i, s)" in text
    assert "visibility_i = (double)(S - count_i) / (double)S, one true division" in text
    assert "AMBIENT OCCLUSION PLANE" in text
    assert text.index("RAY QUERIES, specified") < text.index("AMBIENT OCCLUSION, specified")
    assert int(re.search(r"#define RAYRS_ABI_VERSION (\d+)", header()).group(1)) == 7
    lab = open(os.path.join(ROOT, "rayrs_amd", "csrc", "rayrs_lab.h")).read()
    for name in LAB_SYMBOLS:
        assert re.search(rf"\bint {name}\s*\(", lab), name
    assert "refill_below" not in re.search(r"typedef struct \{(.*?)\} rayrs_lab_tuning;", lab, re.S).group(1)


def test_the_binding_declares_and_the_library_exports_the_entry_points():
    L = _ffi.lib()
    assert L.rayrs_abi_version() == _ffi.ABI_VERSION == 7
    for name in NEW_SYMBOLS:
        assert name in _ffi.SYMBOLS and hasattr(L, name) and getattr(L, name).argtypes, name
    for name in LAB_SYMBOLS:
        assert name in _ffi.PRIVATE_SYMBOLS and hasattr(L, name) and getattr(L, name).argtypes, name
    assert hasattr(rayrs_amd.Scene, "ambient_occlusion") and hasattr(rayrs_amd, "render_ao")
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"fn {name}\(", text), name


def host_scene():
    cam_args, objs, heur, env = _film.sphere_desc()
    return rayrs_amd.Scene(objs, 1e-6, 1e6, heur, env, device=-1), rayrs_amd.Camera(*cam_args)


@pytest.mark.parametrize("n", [4, 0])
def test_refusals_on_a_host_only_scene_come_in_the_headers_order(n):
    """A NULL scene, position or normal, both outputs NULL, samples == 0, fast_traversal > 1 (with n == 0 too, and whatever
    else is wrong beside them), and only then RAYRS_NO_DEVICE; one NULL output is accepted up to RAYRS_NO_DEVICE."""
    L = _ffi.lib()
    scene, cam = host_scene()
    p, nrm = np.zeros((4, 3)), np.ones((4, 3))
    cnt, vis = np.zeros(4, dtype=np.uint32), np.zeros(4)
    P = lambda a: a.ctypes.data

    def ao(launch, scene_h=scene._h, p_=P(p), n_=P(nrm), samples=4, fast=0, cnt_=P(cnt), vis_=P(vis)):
        args = (scene_h, p_, n_, n, samples, float("inf"), 0.0, 1, 0, fast, cnt_, vis_)
        return L.rayrs_scene_ambient_occlusion_launch(*args, None) if launch else L.rayrs_scene_ambient_occlusion(*args)

    for launch in (False, True):
        for bad in (dict(scene_h=None), dict(p_=None), dict(n_=None), dict(cnt_=None, vis_=None), dict(samples=0), dict(fast=2),
                    dict(fast=0xffffffff)):
            assert ao(launch, **bad) == INVALID_ARG, (launch, bad)
            if "fast" not in bad:
                assert ao(launch, fast=2, **bad) == INVALID_ARG
            if "samples" not in bad:
                assert ao(launch, samples=0, **bad) == INVALID_ARG
        assert ao(launch) == NO_DEVICE and ao(launch, fast=1) == NO_DEVICE
        assert ao(launch, cnt_=None) == NO_DEVICE and ao(launch, vis_=None) == NO_DEVICE
    if n:
        with pytest.raises(_ffi.RayrsError) as e:
            scene.ambient_occlusion(p, nrm)
        assert e.value.status == NO_DEVICE

    def plane(scene_h=scene._h, cam_=cam.desc, samples=4, fast=0, cnt_=P(cnt), vis_=P(vis)):
        import ctypes as C
        return L.rayrs_render_ao(scene_h, None if cam_ is None else C.byref(cam_), 1, 2, samples, float("inf"), 0.0, fast, cnt_, vis_)

    for bad in (dict(scene_h=None), dict(cam_=None), dict(cnt_=None, vis_=None), dict(samples=0), dict(fast=2)):
        assert plane(**bad) == INVALID_ARG, bad
    assert plane() == NO_DEVICE and plane(vis_=None) == NO_DEVICE
    assert L.rayrs_lab_ao_refill(None, 1) == INVALID_ARG and L.rayrs_lab_ao_refill(scene._h, 65) == INVALID_ARG
    assert L.rayrs_lab_ao_refill(scene._h, 64) == 0 and L.rayrs_lab_ao_refill(scene._h, 0) == 0


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the wrapper called {name} before it checked its inputs")


def test_the_wrapper_refuses_bad_shapes_before_any_library_call(monkeypatch):
    scene, _ = host_scene()
    monkeypatch.setattr(scene, "_L", NoLibrary())
    good = np.zeros((5, 3))
    for bad_p, bad_n in ((np.zeros((5, 2)), good), (good, np.zeros((4, 3))), (np.zeros(15), np.zeros(15))):
        with pytest.raises(ValueError):
            scene.ambient_occlusion(bad_p, bad_n)
    with pytest.raises(ValueError):
        scene.ambient_occlusion(good, good, samples=0)
    with pytest.raises(AssertionError, match="rayrs_scene_ambient_occlusion"):
        scene.ambient_occlusion(good, good)


# ---- kernel resources.  query_occluded_kernel at the parent commit: 98 registers in the compact layout, 108 in the f64 layout,
# no scratch: 4 waves per SIMD (512 / 128).  ao_kernel's bound is that occupancy class, and no scratch at all -- so none in its walk.
QUERY_OCCLUDED_VGPR = 108
WAVES_PER_SIMD = 512 // 128
AO_VGPR_BOUND = 512 // WAVES_PER_SIMD


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_the_ao_kernels_keep_the_occlusion_querys_occupancy_class(tmp_path):
    res = kernel_resources(compile_asm("ao.hip", tmp_path))
    ao = {n: r for n, r in res.items() if "ao_kernel" in n}
    primary = {n: r for n, r in res.items() if "ao_primary_kernel" in n}
    assert len(ao) == 8 and len(primary) == 2 and len(res) == 10   # COMPACT x EXACT x STEPS; COMPACT
    assert 512 // ((QUERY_OCCLUDED_VGPR + 7) // 8 * 8) == WAVES_PER_SIMD
    for name, (vgpr, scratch, lds) in ao.items():
        # static LDS: 256 counters and the 8-byte cursor; the stacks are dynamic
        assert vgpr <= AO_VGPR_BOUND and scratch == 0 and lds == 256 * 4 + 8, (name, vgpr, scratch, lds)
    for name, (vgpr, scratch, lds) in primary.items():
        assert vgpr <= AO_VGPR_BOUND and scratch == 0 and lds == 0, (name, vgpr, scratch, lds)
