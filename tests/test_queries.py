"""Ray queries (include/rayrs_hip.h RAY QUERIES) without a GPU: the four entry points are declared and exported, every refusal
that is decided before the device is touched comes in the header's order, the Python wrappers refuse bad shapes before any
library call, and the query kernels keep their resources."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _film
import rayrs_amd
from rayrs_amd import _ffi
from test_features import HIPCC, compile_asm, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["rayrs_scene_intersect", "rayrs_scene_occluded", "rayrs_scene_intersect_launch", "rayrs_scene_occluded_launch"]
INVALID_ARG, NO_DEVICE = -1, -4


def header():
    return open(os.path.join(ROOT, "include", "rayrs_hip.h")).read()


def test_the_header_declares_the_entry_points_with_their_contract():
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\bint {name}\s*\(", code), name
    text = re.sub(r"\s*\n \*\s*", " ", header())
    assert "RAY QUERIES, specified to the operation" in text
    assert "occluded_i = 1 iff the closest-hit query above finds a hit and t < t_max_i" in text
    assert "a NaN, zero or negative t_max gives 0" in text
    assert "t_max == NULL means +infinity for every ray" in text
    assert "t_max is never handed to a box test or to the accept rule" in text
    assert "on a miss t = +0, object = 0xFFFFFFFF, normal = (+0, +0, +0)" in text
    assert "fast_traversal = 1 is taken AS ASKED" in text
    assert "the leaf-box bet WITHOUT the culling bet" in text
    assert "at most 2^20 rays each" in text
    assert int(re.search(r"#define RAYRS_ABI_VERSION (\d+)", header()).group(1)) == 7


def test_the_library_exports_the_entry_points():
    L = _ffi.lib()
    assert L.rayrs_abi_version() == _ffi.ABI_VERSION == 7
    for name in NEW_SYMBOLS:
        assert name in _ffi.SYMBOLS and hasattr(L, name), name
    assert hasattr(rayrs_amd.Scene, "intersect") and hasattr(rayrs_amd.Scene, "occluded")


def test_integration_md_has_the_fn_lines():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"fn {name}\(", text), name


def host_scene():
    cam_args, objs, heur, env = _film.sphere_desc()
    return rayrs_amd.Scene(objs, 1e-6, 1e6, heur, env, device=-1)


@pytest.mark.parametrize("n", [4, 0])
def test_refusals_on_a_host_only_scene_come_in_the_headers_order(n):
    """A NULL scene or required buffer (with n == 0 too), then fast_traversal > 1, then RAYRS_NO_DEVICE; NULL normal and NULL
    t_max are accepted up to RAYRS_NO_DEVICE.  The _launch forms refuse alike (a host-only scene has no device pointer to
    give: the refusals never look at what the pointers point to)."""
    L = _ffi.lib()
    scene = host_scene()
    o, d, t_max = np.zeros((4, 3)), np.ones((4, 3)), np.ones(4)
    t, obj, nrm, occ = np.zeros(4), np.zeros(4, dtype=np.uint32), np.zeros((4, 3)), np.zeros(4, dtype=np.uint8)
    P = lambda a: a.ctypes.data

    def intersect(launch, scene_h=scene._h, o_=P(o), d_=P(d), fast=0, t_=P(t), obj_=P(obj), nrm_=P(nrm)):
        if launch:
            return L.rayrs_scene_intersect_launch(scene_h, o_, d_, n, fast, t_, obj_, nrm_, None)
        return L.rayrs_scene_intersect(scene_h, o_, d_, n, fast, t_, obj_, nrm_)

    def occluded(launch, scene_h=scene._h, o_=P(o), d_=P(d), tm_=P(t_max), fast=0, occ_=P(occ)):
        if launch:
            return L.rayrs_scene_occluded_launch(scene_h, o_, d_, tm_, n, fast, occ_, None)
        return L.rayrs_scene_occluded(scene_h, o_, d_, tm_, n, fast, occ_)

    for launch in (False, True):
        for missing in ("scene_h", "o_", "d_", "t_", "obj_"):
            assert intersect(launch, **{missing: None}) == INVALID_ARG, (launch, missing)
            assert intersect(launch, fast=2, **{missing: None}) == INVALID_ARG
        for missing in ("scene_h", "o_", "d_", "occ_"):
            assert occluded(launch, **{missing: None}) == INVALID_ARG, (launch, missing)
        assert intersect(launch, fast=2) == INVALID_ARG and occluded(launch, fast=2) == INVALID_ARG
        assert intersect(launch, fast=0xffffffff) == INVALID_ARG
        # everything in order: the scene has no device
        assert intersect(launch) == NO_DEVICE and intersect(launch, fast=1) == NO_DEVICE
        assert occluded(launch) == NO_DEVICE and occluded(launch, fast=1) == NO_DEVICE
        assert intersect(launch, nrm_=None) == NO_DEVICE
        assert occluded(launch, tm_=None) == NO_DEVICE
    with pytest.raises(_ffi.RayrsError) as e:
        scene.intersect(o, d)
    assert e.value.status == NO_DEVICE
    with pytest.raises(_ffi.RayrsError) as e:
        scene.occluded(o, d, t_max)
    assert e.value.status == NO_DEVICE


class NoLibrary:
    """Stands in for the loaded library: a wrapper that reaches it has not refused its inputs first."""

    def __getattr__(self, name):
        raise AssertionError(f"the wrapper called {name} before it checked its inputs")


def test_the_wrappers_refuse_bad_shapes_before_any_library_call(monkeypatch):
    scene = host_scene()
    monkeypatch.setattr(scene, "_L", NoLibrary())
    good = np.zeros((5, 3))
    for call in (scene.intersect, scene.occluded):
        with pytest.raises(ValueError):
            call(np.zeros((5, 2)), good)
        with pytest.raises(ValueError):
            call(good, np.zeros((5, 2)))
        with pytest.raises(ValueError):
            call(good, np.zeros((4, 3)))
        with pytest.raises(ValueError):
            call(np.zeros(15), np.zeros(15))
        with pytest.raises(ValueError):
            call(np.zeros((5, 3, 1)), good)
    for bad in (np.zeros(4), np.zeros(6), np.zeros((5, 1)), np.float64(1.0)):
        with pytest.raises(ValueError):
            scene.occluded(good, good, t_max=bad)
    # and a good call does reach the library
    with pytest.raises(AssertionError, match="rayrs_scene_occluded"):
        scene.occluded(good, good, t_max=np.ones(5))
    with pytest.raises(AssertionError, match="rayrs_scene_intersect"):
        scene.intersect([[0.0, 0.0, 0.0]], [[0.0, 0.0, 1.0]], normals=True)


def test_torch_tensors_off_the_scenes_gpu_are_refused_before_any_library_call(monkeypatch):
    """No GPU here: a CPU tensor is a tensor on the wrong device, alone or beside numpy arrays, whatever its dtype."""
    torch = pytest.importorskip("torch")
    scene = host_scene()
    monkeypatch.setattr(scene, "_L", NoLibrary())
    good = np.zeros((5, 3))
    for dtype in (torch.float64, torch.float32):
        cpu = torch.zeros((5, 3), dtype=dtype)
        for call in (scene.intersect, scene.occluded):
            with pytest.raises(ValueError):
                call(cpu, cpu)
            with pytest.raises(ValueError):
                call(good, cpu)
    with pytest.raises(ValueError):
        scene.occluded(good, good, t_max=torch.ones(5, dtype=torch.float64))


needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@needs_hipcc
def test_the_query_kernels_keep_their_occupancy_class(tmp_path):
    """Each query on the compact and on the f64 layout, the occlusion query also in the lab's step-counting instance.  At most
    128 registers (4 waves per SIMD) -- the compact closest-hit kernel at most 96 (5) -- no scratch, and no LDS but the
    traversal stacks they are launched with."""
    res = kernel_resources(compile_asm("query.hip", tmp_path))
    assert len(res) == 6
    assert sum("query_intersect_kernel" in n for n in res) == 2 and sum("query_occluded_kernel" in n for n in res) == 4
    for name, (vgpr, scratch, lds) in res.items():
        bound = 96 if "query_intersect_kernelILb1E" in name else 128
        assert vgpr <= bound and scratch == 0 and lds == 0, (name, vgpr, scratch, lds)
