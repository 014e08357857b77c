"""The direct-lit films (include/rayrs_hip.h DIRECT-LIT FILMS) without a GPU: the header states the contract, the two entry points
are declared, exported and bound, Film refuses its arguments before it needs a device, every refusal of a creation that is
decided before the device is touched comes in the header's order, film_direct.hip's kernels keep the resources of the waves they
run, and the expectation the GPU tests fold from the readings' per-sample values is the readings' own answer."""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest

import _film
import _film_direct as FD
import _sky
import rayrs_amd
from rayrs_amd import SKY, _ffi, scenes
from test_features import HIPCC, compile_asm, kernel_resources
from test_sky import MAPS, host_scene, room_scene, scene_names
import _lit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["rayrs_film_create_direct", "rayrs_film_create_sky"]
INVALID_ARG, NO_DEVICE, UNSUPPORTED = -1, -4, -5


def header():
    return open(os.path.join(ROOT, "include", "rayrs_hip.h")).read()


def test_the_header_states_the_contract_and_the_binding_declares_the_entry_points():
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(rf"\bint {name}\s*\(", code), name
    text = re.sub(r"\s+", " ", re.sub(r"\s*\n \*\s*", " ", header()))
    assert text.index("SKY SAMPLING, specified") < text.index("DIRECT-LIT FILMS.") < text.index("The boundary's version")
    assert "THE CONTRACT and THE CONTRACT PER TILE of the progressive film hold word for word with rayrs_render_direct (rayrs_render_sky)" in text
    assert "the light list is NOT recorded in it" in text and "is the caller's error" in text
    assert "c * (2 * max_bounces + 1) >= 2^32" in text and "ceil(n / c) * 64 <= 2^20" in text
    assert int(re.search(r"#define RAYRS_ABI_VERSION (\d+)", header()).group(1)) == 7
    L = _ffi.lib()
    assert L.rayrs_abi_version() == _ffi.ABI_VERSION == 7
    vp = C.c_void_p
    for name in ENTRY_POINTS:
        assert name in _ffi.SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).argtypes == [vp, C.POINTER(_ffi.CameraDesc), C.POINTER(_ffi.FilmParams), vp, C.c_uint32, C.POINTER(vp)], name
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRY_POINTS:
        assert re.search(rf"fn {name}\(", doc), name


def small_camera():
    return rayrs_amd.Camera(*scenes.camera_for_resolution(_lit.lit_room()[0], 16, 8))


def test_film_refuses_its_arguments_without_a_device():
    scene, cam = room_scene(MAPS["studio"]), small_camera()
    with pytest.raises(ValueError):
        rayrs_amd.Film(scene, cam, direct=True)
    with pytest.raises(ValueError):
        rayrs_amd.Film(scene, cam, lights=[3, 4])
    with pytest.raises(ValueError):
        rayrs_amd.Film(scene, cam, lights=[])
    with pytest.raises(ValueError):
        rayrs_amd.Film(scene, cam, lights=[-1], direct=True)
    # what reaches the library is refused there, by the entry point the list chooses: the scene has no device
    for lights in ([3, 4], [], [SKY], [3, SKY, 4], [SKY, SKY]):
        with pytest.raises(_ffi.RayrsError) as e:
            rayrs_amd.Film(scene, cam, lights=lights, direct=True)
        assert e.value.status == NO_DEVICE, lights
    with pytest.raises(_ffi.RayrsError) as e:   # (the _direct call refuses the sky's number as an index; the _sky call never sees it)
        rayrs_amd.Film(scene, cam, lights=[100], direct=True)
    assert e.value.status == INVALID_ARG
    black = room_scene(np.zeros((5, 9, 3), dtype=np.float32))
    with pytest.raises(_ffi.RayrsError) as e:
        rayrs_amd.Film(black, cam, lights=[SKY], direct=True)
    assert e.value.status == UNSUPPORTED
    with pytest.raises(_ffi.RayrsError) as e:
        rayrs_amd.Film(black, cam, lights=[3], direct=True)
    assert e.value.status == NO_DEVICE


def test_refusals_at_creation_come_in_the_headers_order():
    """On the host-only room with a triangle and the material rule's spheres (tests/test_sky.py host_scene), under a lit and under
    a black sky: each condition alone, and beside one of a later group."""
    L = _ffi.lib()
    scene, tri = host_scene(MAPS["studio"])
    black, _ = host_scene(np.zeros((5, 9, 3), dtype=np.float32))
    N = scene_names
    cam = small_camera()
    u32 = lambda *v: np.array(v, dtype=np.uint32)
    good, nine = u32(3, 4, 5), u32(3, 4, 5, 3, 4, 5, 3, 4, 5)

    def desc(**fields):
        d = copy.copy(cam.desc)
        for k, v in fields.items():
            setattr(d, k, v)
        return d

    def call(sky, sc, lights=good, n_lights=None, cam_=None, no_scene=False, no_cam=False, no_params=False, no_out=False, chunk=2,
             bounces=50, rank=0, ranks=1, fast=0, pad=0):
        p = _ffi.FilmParams()
        p.sample_chunk, p.max_bounces, p.seed, p.tile_rank, p.tile_ranks, p.fast_traversal, p.pad = chunk, bounces, 1, rank, ranks, fast, pad
        d = cam.desc if cam_ is None else cam_
        h = C.c_void_p()
        nl = (0 if lights is None else len(lights)) if n_lights is None else n_lights
        f = L.rayrs_film_create_sky if sky else L.rayrs_film_create_direct
        st = f(None if no_scene else sc._h, None if no_cam else C.byref(d), None if no_params else C.byref(p),
               None if lights is None or len(lights) == 0 else lights.ctypes.data, nl, None if no_out else C.byref(h))
        assert not h.value
        return st

    invalid = (dict(no_scene=True), dict(no_cam=True), dict(no_params=True), dict(no_out=True), dict(rank=1), dict(rank=2, ranks=2),
               dict(fast=2), dict(pad=1), dict(cam_=desc(x_pixels=0)), dict(cam_=desc(y_pixels=0)),
               dict(lights=None, n_lights=3), dict(lights=u32(3, 100)), dict(lights=u32(0xffffffff)), dict(lights=u32(N["plastic_lamp"], 100)))
    unsupported = (dict(cam_=desc(x_pixels=65536)), dict(bounces=8001), dict(chunk=1 << 30), dict(lights=nine), dict(lights=u32(3, tri)),
                   dict(lights=u32(tri)), dict(lights=u32(N["plastic_lamp"])), dict(lights=u32(N["noreflect_lamp"])),
                   dict(lights=u32(N["refract_lamp"])), dict(lights=u32(3, 4, N["plastic_lamp"], 5)),
                   dict(chunk=1 << 20, bounces=2048))   # 2^20 * 4097 >= 2^32
    later = (dict(bounces=8001), dict(chunk=1 << 30))
    ok = (dict(), dict(fast=1), dict(ranks=2), dict(rank=1, ranks=2), dict(lights=None), dict(lights=u32(), n_lights=0),
          dict(lights=u32(3, 3, 3, 3, 4, 4, 4, 4)), dict(lights=u32(0, 1, 2)), dict(lights=u32(N["plastic_dark"])),
          dict(lights=u32(N["noreflect_dark"], 3)), dict(lights=u32(N["glass_lamp"])), dict(chunk=1 << 20, bounces=2047), dict(bounces=0))
    for sky in (False, True):
        for sc in (scene, black):
            for bad in invalid:
                assert call(sky, sc, **bad) == INVALID_ARG, (sky, bad)
                for more in later:
                    assert call(sky, sc, **bad, **more) == INVALID_ARG, (sky, bad, more)
                if "lights" not in bad:
                    assert call(sky, sc, lights=nine, **bad) == INVALID_ARG, (sky, bad)
                    assert call(sky, sc, lights=u32(tri), **bad) == INVALID_ARG, (sky, bad)
            for big in unsupported:
                assert call(sky, sc, **big) == UNSUPPORTED, (sky, big)
        for good_call in ok:
            assert call(sky, scene, **good_call) == NO_DEVICE, (sky, good_call)
            # the empty table is the sky film's refusal alone, after the material rule and before the device
            assert call(sky, black, **good_call) == (UNSUPPORTED if sky else NO_DEVICE), (sky, good_call)
    # the plain film's creation is as it was
    p = _ffi.FilmParams()
    p.sample_chunk, p.max_bounces = 2, 50
    h = C.c_void_p()
    assert L.rayrs_film_create(scene._h, C.byref(cam.desc), C.byref(p), C.byref(h)) == NO_DEVICE


# ---- kernel resources: what the direct and the sky kernels are held to (tests/test_direct.py, tests/test_sky.py)
VGPR_BOUND = 256


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_the_film_kernels_use_no_scratch_and_keep_two_waves_per_simd(tmp_path):
    res = kernel_resources(compile_asm("film_direct.hip", tmp_path))
    direct = {n: r for n, r in res.items() if "film_direct_kernel" in n}
    sky = {n: r for n, r in res.items() if "film_sky_kernel" in n}
    count = {n: r for n, r in res.items() if "film_direct_count_kernel" in n}
    assert len(direct) == 4 and len(sky) == 4 and len(count) == 1 and len(res) == 9   # COMPACT x EXACT of either wave; the counts
    for name, (vgpr, scratch, lds) in res.items():
        print(name, vgpr, scratch, lds)
        assert vgpr <= VGPR_BOUND and scratch == 0 and lds == 0, (name, vgpr, scratch, lds)   # (the stacks are dynamic LDS)


# ---- the GPU tests' expectation is the readings' own

@pytest.mark.parametrize("kernel", FD.KERNELS)
def test_the_folded_expectation_is_the_readings_answer(kernel):
    """_film.expectation over the per-sample values, N = 6 in chunks of 2, and _sky.answers (= _direct.answers) over the same
    values: one frame, bit for bit, and the query counts the films' `rays` are summed from."""
    rgb, q = FD.paths("room", kernel)
    assert rgb.shape == (FD.H, FD.W, FD.N_MAX, 3) and q.shape == (FD.H, FD.W, FD.N_MAX) and np.isfinite(rgb).all()
    frame = _film.expectation(rgb, 2, 6)[0]
    values, queries = rgb.reshape(-1, FD.N_MAX, 3)[:, :6], q.reshape(-1, FD.N_MAX)[:, :6].astype(np.int64)
    want, want_q = _sky.answers(values, queries, 2)
    assert np.array_equal(frame.reshape(-1, 3).view(np.uint64), np.ascontiguousarray(want).view(np.uint64))
    assert int(q[:, :, :6].sum()) == int(want_q.sum(dtype=np.uint64)) and (q >= 1).all()
