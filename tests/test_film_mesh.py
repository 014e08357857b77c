"""The mesh-lit films and bakes (include/rayrs_hip.h MESH-LIT FILMS AND BAKES) without a GPU: the two entry points are declared,
exported and bound, every refusal of either creation comes in the header's order on host-only scenes, Film and Bake refuse a
group without direct=True before they need a device, and film_mesh.hip's and bake_mesh.hip's kernels keep the resources of the
wave they run."""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest

import _lit
import rayrs_amd
from rayrs_amd import SKY, _ffi, procedural, scenes
from rayrs_amd.api import Emission, Material, Object
from test_mesh_lights import HIPCC, compile_asm, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, NO_DEVICE, UNSUPPORTED = -1, -4, -5
STUDIO = procedural.make_studio_hdri(9, 5)
BLACK = np.zeros((5, 9, 3), dtype=np.float32)
Z_NEAR, Z_FAR = 1e-6, 1e6
TRI_A, TRI_B, PLASTIC_LAMP, PLASTIC_DARK = 6, 7, 8, 9


def host_scene(hdri=STUDIO):
    """The lit room's objects 0..5 (3, 4, 5 are legal lamps), two emissive Lambertian triangles (6, 7), an emissive Plastic sphere
    (8: the material rule refuses it) and a dark Plastic one (9: legal), host-only."""
    cam, objs, heur, names = _lit.lit_room()
    white, glow = Material.LambertianDiffuse((0.8, 0.8, 0.8)), Emission.new(4.0, (1.0, 0.9, 0.8))
    plastic = Material.Plastic((0.7, 0.2, 0.2), (1.0, 1.0, 1.0), 0.2, 1.5)
    objs = list(objs)
    assert len(objs) == 6
    objs += [Object.triangle((-3.0, 3.0, 0.0), (-2.5, 3.0, 0.0), (-3.0, 3.0, 0.5), white, glow),
             Object.triangle((-2.0, 3.0, 0.0), (-1.5, 3.0, 0.0), (-2.0, 3.0, 0.5), white, glow),
             Object.sphere(0.1, (3.0, 0.2, -3.0), plastic, glow), Object.sphere(0.1, (3.0, 0.2, -2.5), plastic, Emission.Dark())]
    return rayrs_amd.Scene(objs, Z_NEAR, Z_FAR, heur, hdri, device=-1)


def small_camera():
    return rayrs_amd.Camera(*scenes.camera_for_resolution(_lit.lit_room()[0], 16, 8))


def u32(*v):
    return np.array(v, dtype=np.uint32)


GOOD, NINE = u32(3, 4, 5), u32(3, 4, 5, 3, 4, 5, 3, 4, 5)


def test_the_header_states_the_contract_and_the_binding_declares_the_entry_points():
    head = open(os.path.join(ROOT, "include", "rayrs_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", head, flags=re.S)
    for name in ("rayrs_film_create_mesh", "rayrs_bake_create_mesh"):
        assert re.search(rf"\bint {name}\s*\(", code), name
    text = re.sub(r"\s+", " ", re.sub(r"\s*\n \*\s*", " ", head))
    assert text.index("BAKE. The progressive film's machinery") < text.index("MESH-LIT FILMS AND BAKES.") < text.index("The boundary's version")
    assert "the group is NOT recorded, as the list is not" in text and "BORROWS the group" in text
    assert int(re.search(r"#define RAYRS_ABI_VERSION (\d+)", head).group(1)) == 7
    L = _ffi.lib()
    vp = C.c_void_p
    for name in ("rayrs_film_create_mesh", "rayrs_bake_create_mesh"):
        assert name in _ffi.SYMBOLS and hasattr(L, name), name
    assert L.rayrs_film_create_mesh.argtypes == [vp, C.POINTER(_ffi.CameraDesc), C.POINTER(_ffi.FilmParams), vp, C.c_uint32, vp, C.c_uint32,
                                                 C.POINTER(vp)]
    assert L.rayrs_bake_create_mesh.argtypes == [vp, vp, vp, C.c_uint64, C.POINTER(_ffi.BakeParams), vp, C.c_uint32, vp, C.POINTER(vp)]


def test_the_films_refusals_at_creation_come_in_the_headers_order():
    """rayrs_film_create_direct's refusals in their order (sky = 1: rayrs_film_create_sky's), a handle of another scene and a sky
    above 1 in the RAYRS_INVALID_ARG group, RAYRS_NO_DEVICE last -- with a group, with an empty one and with none, each condition
    alone and beside one of a later group."""
    L = _ffi.lib()
    scene, other, black = host_scene(), host_scene(), host_scene(BLACK)
    mesh, empty, foreign, on_black = scene.mesh_lights([TRI_A, TRI_B]), scene.mesh_lights([]), other.mesh_lights([TRI_A]), black.mesh_lights([TRI_A])
    cam = small_camera()

    def desc(**fields):
        d = copy.copy(cam.desc)
        for k, v in fields.items():
            setattr(d, k, v)
        return d

    def call(sky, sc=scene, m=mesh, lights=GOOD, n_lights=None, cam_=None, no_scene=False, no_cam=False, no_params=False, no_out=False,
             chunk=2, bounces=50, rank=0, ranks=1, fast=0, pad=0):
        p = _ffi.FilmParams()
        p.sample_chunk, p.max_bounces, p.seed, p.tile_rank, p.tile_ranks, p.fast_traversal, p.pad = chunk, bounces, 1, rank, ranks, fast, pad
        d = cam.desc if cam_ is None else cam_
        h = C.c_void_p()
        nl = (0 if lights is None else len(lights)) if n_lights is None else n_lights
        st = L.rayrs_film_create_mesh(None if no_scene else sc._h, None if no_cam else C.byref(d), None if no_params else C.byref(p),
                                      None if lights is None or len(lights) == 0 else lights.ctypes.data, nl, None if m is None else m._h,
                                      int(sky), None if no_out else C.byref(h))
        assert not h.value
        return st

    invalid = (dict(no_scene=True), dict(no_cam=True), dict(no_params=True), dict(no_out=True), dict(rank=1), dict(rank=2, ranks=2),
               dict(fast=2), dict(pad=1), dict(cam_=desc(x_pixels=0)), dict(cam_=desc(y_pixels=0)),
               dict(lights=None, n_lights=3), dict(lights=u32(3, 100)), dict(lights=u32(0xffffffff)), dict(lights=u32(PLASTIC_LAMP, 100)))
    unsupported = (dict(cam_=desc(x_pixels=65536)), dict(bounces=8001), dict(chunk=1 << 30), dict(lights=NINE), dict(lights=u32(3, TRI_A)),
                   dict(lights=u32(TRI_B)), dict(lights=u32(PLASTIC_LAMP)), dict(lights=u32(3, 4, PLASTIC_LAMP, 5)),
                   dict(chunk=1 << 20, bounces=2048))   # the 32-bit counter rule: 2^20 * 4097 >= 2^32
    later = (dict(bounces=8001), dict(chunk=1 << 30), dict(lights=u32(TRI_A)), dict(lights=u32(PLASTIC_LAMP)))
    ok = (dict(), dict(fast=1), dict(rank=1, ranks=2), dict(lights=None), dict(lights=u32(), n_lights=0), dict(lights=u32(3, 3, 3, 3, 4, 4, 4, 4)),
          dict(lights=u32(PLASTIC_DARK)), dict(chunk=1 << 20, bounces=2047), dict(bounces=0))
    for sky in (0, 1):
        for m in (mesh, empty, None):
            for bad in invalid:
                assert call(sky, m=m, **bad) == INVALID_ARG, (sky, bad)
                for more in later:
                    if not ("lights" in bad and "lights" in more):
                        assert call(sky, m=m, **bad, **more) == INVALID_ARG, (sky, bad, more)
            for big in unsupported:
                assert call(sky, m=m, **big) == UNSUPPORTED, (sky, big)
            for good_call in ok:
                assert call(sky, m=m, **good_call) == NO_DEVICE, (sky, good_call)
        # a handle of another scene: RAYRS_INVALID_ARG, before everything of the RAYRS_UNSUPPORTED group
        for extra in (dict(), dict(bounces=8001), dict(lights=u32(TRI_A)), dict(lights=u32(PLASTIC_LAMP)), dict(cam_=desc(x_pixels=65536))):
            assert call(sky, m=foreign, **extra) == INVALID_ARG, (sky, extra)
    # a sky above 1: RAYRS_INVALID_ARG, beside anything of a later group
    for m in (mesh, empty, None, foreign):
        for extra in (dict(), dict(bounces=8001), dict(lights=u32(TRI_A)), dict(chunk=1 << 20, bounces=2048)):
            assert call(2, m=m, **extra) == INVALID_ARG, extra
            assert call(0xffffffff, m=m, **extra) == INVALID_ARG, extra
    # the all-black map: the sky film's refusal alone, after the rest of the RAYRS_UNSUPPORTED group and before the device
    for m in (on_black, None):
        assert call(0, sc=black, m=m) == NO_DEVICE
        assert call(1, sc=black, m=m) == UNSUPPORTED
        assert call(1, sc=black, m=m, lights=None) == UNSUPPORTED
        assert call(1, sc=black, m=m, fast=2) == INVALID_ARG
    assert call(1, sc=black, m=mesh) == INVALID_ARG   # (another scene's handle comes first)
    for h in (mesh, empty, foreign, on_black):
        h.close()


def test_the_bakes_refusals_at_creation_come_in_the_headers_order():
    """rayrs_bake_create's refusals in their order, a handle of another scene in the RAYRS_INVALID_ARG group, the counter rule of a
    bake with a group, RAYRS_NO_DEVICE last."""
    L = _ffi.lib()
    scene, other, black = host_scene(), host_scene(), host_scene(BLACK)
    mesh, empty, foreign, on_black = scene.mesh_lights([TRI_A, TRI_B]), scene.mesh_lights([]), other.mesh_lights([TRI_A]), black.mesh_lights([TRI_A])
    pts = np.zeros((4, 3))

    def call(sky, sc=scene, m=mesh, lights=GOOD, n_lights=None, n=4, no_scene=False, no_a=False, no_b=False, no_params=False, no_out=False,
             kind=0, chunk=2, bounces=50, fast=0, pad=0):
        p = _ffi.BakeParams()
        p.kind, p.sample_chunk, p.max_bounces, p.fast_traversal, p.seed, p.pad, p.sky = kind, chunk, bounces, fast, 1, pad, sky
        h = C.c_void_p()
        nl = (0 if lights is None else len(lights)) if n_lights is None else n_lights
        st = L.rayrs_bake_create_mesh(None if no_scene else sc._h, None if no_a else pts.ctypes.data, None if no_b else pts.ctypes.data, n,
                                      None if no_params else C.byref(p), None if lights is None or len(lights) == 0 else lights.ctypes.data,
                                      nl, None if m is None else m._h, None if no_out else C.byref(h))
        assert not h.value
        return st

    invalid = (dict(no_scene=True), dict(no_a=True), dict(no_b=True), dict(no_params=True), dict(no_out=True), dict(fast=2), dict(pad=1),
               dict(kind=2), dict(lights=None, n_lights=3), dict(lights=u32(3, 100)), dict(lights=u32(0xffffffff)),
               dict(lights=u32(PLASTIC_LAMP, 100)))
    unsupported = (dict(bounces=8001), dict(chunk=1 << 30), dict(lights=NINE), dict(lights=u32(3, TRI_A)), dict(lights=u32(TRI_B)),
                   dict(lights=u32(PLASTIC_LAMP)), dict(lights=u32(3, 4, PLASTIC_LAMP, 5)), dict(chunk=1 << 20, bounces=2048),
                   dict(n=1 << 32))
    later = (dict(bounces=8001), dict(chunk=1 << 30), dict(n=1 << 32))
    ok = (dict(), dict(fast=1), dict(kind=1), dict(n=0), dict(n=(1 << 32) - 1), dict(lights=u32(3, 3, 3, 3, 4, 4, 4, 4)),
          dict(lights=u32(PLASTIC_DARK)), dict(chunk=1 << 20, bounces=2047), dict(chunk=0), dict(bounces=0))
    for sky in (0, 1):
        for m in (mesh, empty, None):
            for bad in invalid:
                assert call(sky, m=m, **bad) == INVALID_ARG, (sky, bad)
                for more in later:
                    assert call(sky, m=m, **bad, **more) == INVALID_ARG, (sky, bad, more)
            for big in unsupported:
                assert call(sky, m=m, **big) == UNSUPPORTED, (sky, big)
            for good_call in ok:
                assert call(sky, m=m, **good_call) == NO_DEVICE, (sky, good_call)
        for extra in (dict(), dict(bounces=8001), dict(lights=u32(TRI_A)), dict(n=1 << 32)):
            assert call(sky, m=foreign, **extra) == INVALID_ARG, (sky, extra)
    for m in (mesh, empty, None, foreign):
        assert call(2, m=m) == INVALID_ARG and call(2, m=m, bounces=8001) == INVALID_ARG
    for m in (on_black, None):
        assert call(0, sc=black, m=m) == NO_DEVICE and call(1, sc=black, m=m) == UNSUPPORTED
        assert call(1, sc=black, m=m, kind=2) == INVALID_ARG
    # the counter: without a list, a sky or a group the bake is the unlit one and counts max_bounces queries a sample; a group of
    # N >= 1 triangles has shadow rays, 2 * max_bounces + 1
    none = dict(lights=None, chunk=1 << 20)
    for m in (empty, None):
        assert call(0, m=m, bounces=2048, **none) == NO_DEVICE
        assert call(0, m=m, bounces=4095, **none) == NO_DEVICE
        assert call(0, m=m, bounces=4096, **none) == UNSUPPORTED
        assert call(1, m=m, bounces=2048, **none) == UNSUPPORTED
    assert call(0, m=mesh, bounces=2047, **none) == NO_DEVICE
    assert call(0, m=mesh, bounces=2048, **none) == UNSUPPORTED
    # rayrs_bake_create is as it was
    p = _ffi.BakeParams()
    p.sample_chunk, p.max_bounces = 2, 50
    h = C.c_void_p()
    assert L.rayrs_bake_create(scene._h, pts.ctypes.data, pts.ctypes.data, 4, C.byref(p), None, 0, C.byref(h)) == NO_DEVICE
    for h in (mesh, empty, foreign, on_black):
        h.close()


def test_film_and_bake_refuse_a_group_without_direct_and_hand_the_rest_to_the_library():
    scene, cam = host_scene(), small_camera()
    mesh = scene.mesh_lights([TRI_A, TRI_B])
    pts = np.zeros((4, 3))
    for kw in (dict(), dict(lights=[3])):
        with pytest.raises(ValueError):
            rayrs_amd.Film(scene, cam, mesh=mesh, **kw)
        with pytest.raises(ValueError):
            rayrs_amd.Bake(scene, pts, pts, mesh=mesh, **kw)
    with pytest.raises(ValueError):   # (direct=True still needs a list, which may be empty)
        rayrs_amd.Film(scene, cam, direct=True, mesh=mesh)
    with pytest.raises(ValueError):
        rayrs_amd.Bake(scene, pts, pts, direct=True, mesh=mesh)
    # what reaches the library is refused there, by the mesh creators: the scene has no device
    for lights in ([], [3, 4], [SKY], [3, SKY]):
        with pytest.raises(_ffi.RayrsError) as e:
            rayrs_amd.Film(scene, cam, lights=lights, direct=True, mesh=mesh)
        assert e.value.status == NO_DEVICE and "rayrs_film_create_mesh" in str(e.value), (lights, str(e.value))
        with pytest.raises(_ffi.RayrsError) as e:
            rayrs_amd.Bake(scene, pts, pts, lights=lights, direct=True, mesh=mesh)
        assert e.value.status == NO_DEVICE and "rayrs_bake_create_mesh" in str(e.value), (lights, str(e.value))
    with pytest.raises(_ffi.RayrsError) as e:
        rayrs_amd.Film(scene, cam, lights=[TRI_A], direct=True, mesh=mesh)
    assert e.value.status == UNSUPPORTED
    other = host_scene()
    with pytest.raises(_ffi.RayrsError) as e:
        rayrs_amd.Film(other, cam, lights=[], direct=True, mesh=mesh)
    assert e.value.status == INVALID_ARG
    # mesh=None goes where it went before
    with pytest.raises(_ffi.RayrsError) as e:
        rayrs_amd.Film(scene, cam, lights=[SKY], direct=True)
    assert e.value.status == NO_DEVICE and "rayrs_film_create_sky" in str(e.value)
    with pytest.raises(_ffi.RayrsError) as e:
        rayrs_amd.Bake(scene, pts, pts, lights=[3], direct=True)
    assert e.value.status == NO_DEVICE and "rayrs_bake_create_mesh" not in str(e.value)
    mesh.close()
    with pytest.raises(ValueError):   # a closed group
        rayrs_amd.Film(scene, cam, lights=[], direct=True, mesh=mesh)
    # a group whose scene is closed already drops its handle without a call into the library (interpreter exit finalizes in any order)
    late = other.mesh_lights([TRI_A])
    other.close()
    late.close()
    assert late._h is None


# ---- kernel resources: registers, scratch and LDS, the bound tests/test_mesh_lights.py holds the query kernels to
VGPR_BOUND = 256


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("unit,kernel,count", [("film_mesh.hip", "film_mesh_kernel", 8), ("bake_mesh.hip", "bake_mesh_kernel", 16)])
def test_the_pass_kernels_use_no_scratch_and_keep_two_waves_per_simd(unit, kernel, count, tmp_path):
    res = kernel_resources(compile_asm(unit, tmp_path))
    assert len(res) == count and all(kernel in n for n in res), sorted(res)   # COMPACT x EXACT x SKY (x the bake's two kinds)
    for name, (vgpr, scratch, lds) in sorted(res.items()):
        print(name, vgpr, scratch, lds)
        assert vgpr <= VGPR_BOUND and scratch == 0 and lds == 0, (name, vgpr, scratch, lds)   # (the stacks are dynamic LDS)
