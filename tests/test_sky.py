"""The sky as a light of direct lighting (include/rayrs_hip.h SKY SAMPLING) without a GPU: the header states the operation, the entry
points are declared, exported and bound, the table, sky_sample and p_env of the library's host calls are the plain-Python
reading's (tests/_sky.py) bit for bit, p_env is the density of sky_sample's draws, every refusal that is decided before the device
is touched comes in the header's order -- the empty table among them --, the kernels keep their resources, and the reading of the
turn is held to what makes it worth comparing with: its irradiance has the unlit mean, with lamps beside the sky and with the sky
alone, and the paths of a small image take every branch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _direct
import _lit
import _oracle
import _sky
import rayrs_amd
from rayrs_amd import SKY, _ffi, procedural, scenes
from rayrs_amd.api import Emission, Material, Object
from test_features import HIPCC, compile_asm, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["rayrs_scene_radiance_sky", "rayrs_scene_radiance_sky_launch", "rayrs_scene_irradiance_sky",
                "rayrs_scene_irradiance_sky_launch", "rayrs_render_sky"]
HOST_CALLS = ["rayrs_scene_sky_table", "rayrs_scene_sky_sample", "rayrs_scene_sky_density"]
INVALID_ARG, NO_DEVICE, UNSUPPORTED = -1, -4, -5
Z_NEAR, Z_FAR = 1e-6, 1e6
F = np.float64
# the three maps of the table tests: bright everywhere; black but for two rectangles, with a zero row of cells, zero cells and
# texels at the clip value 3; one cell, with a texel above the clip value
TWO_BY_TWO = np.array([[[0.5, 1.0, 2.0], [0.0, 0.0, 0.0]], [[4.0, 0.125, 0.25], [1.0, 1.0, 1.0]]], dtype=np.float32)
MAPS = {"gradient": procedural.make_hdri(32, 16), "studio": procedural.make_studio_hdri(9, 5), "two_by_two": TWO_BY_TWO}


def header():
    return open(os.path.join(ROOT, "include", "rayrs_hip.h")).read()


def room_scene(hdri):
    cam, objs, heur, names = _lit.lit_room()
    return rayrs_amd.Scene(objs, Z_NEAR, Z_FAR, heur, hdri, device=-1)


def test_the_header_states_the_operation():
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in ENTRY_POINTS + HOST_CALLS:
        assert re.search(rf"\bint {name}\s*\(", code), name
    text = re.sub(r"\s+", " ", re.sub(r"\s*\n \*\s*", " ", header()))
    assert "SKY SAMPLING, specified to the operation" in text
    assert text.index("DIRECT LIGHTING, specified") < text.index("SKY SAMPLING, specified")
    assert "L(i, j) = (r + g) + b of texel(i, j)" in text
    assert "s_i = rr_sin(((double)i + 0.5) * RR_PI / (double)(h - 1))" in text
    assert "A[i][j] = s_i * (((L(i,j) + L(i+1,j)) + L(i,j+1)) + L(i+1,j+1))" in text
    assert "the first assigned, then one add per cell" in text and "R_i = C[i][w-2]" in text and "T = M[h-2]" in text
    assert "T not > 0.0, or not finite, is RAYRS_UNSUPPORTED" in text
    assert "ty = u1 * T; i = the first index with M[i] > ty, or h-2 if there is none" in text
    assert "below = i > 0 ? M[i-1] : 0.0; y = (double)i + (ty - below) / R_i" in text
    assert "tx = u2 * R_i; j = the first index with C[i][j] > tx, or w-2 if there is none" in text
    assert "below = j > 0 ? C[i][j-1] : 0.0; x = (double)j + (tx - below) / A[i][j]" in text
    assert "theta = y / (double)(h - 1) * RR_PI; phi = x / (double)(w - 1) * (2.0 * RR_PI); psi = phi - RR_PI" in text
    assert "l_s = (cp * st, ct, sp * st)" in text
    assert "i = min(usize(floor(y)), h - 2); j = min(usize(floor(x)), w - 2)" in text
    assert "sn = rr_sqrt(1.0 - dir.y * dir.y)" in text
    assert "p_env = ((A[i][j] / T) * ((double)(w - 1) * (double)(h - 1))) / (((2.0 * RR_PI) * RR_PI) * sn)" in text
    assert "a set of measure zero" in text
    assert "k = min((uint32)(b * (double)M), M - 1); l_s = sky_sample(u1, u2) if k == K" in text
    assert "then += p_env(l) last; with K = 0, p_env assigned) / (double)M" in text
    assert "if hit_s is Miss: light = light + (throughput * C) * background(l_s)" in text
    assert "w_next = pc / (pc + pm) if pm > 0.0 else 1.0" in text
    assert "return light + throughput * (background(dir) * w)" in text
    assert "Why it is unbiased" in text and "p_M / (p_M + pc) and by the continuation with weight pc / (p_M + pc)" in text
    assert "n_lights == 0 is legal, the sky alone" in text
    assert "the empty table in the RAYRS_UNSUPPORTED group after the material rule" in text
    assert int(re.search(r"#define RAYRS_ABI_VERSION (\d+)", header()).group(1)) == 7
    assert "rayrs_scene_sky_density (SKY SAMPLING)" in text   # (the version comment)


def test_the_binding_declares_and_the_library_exports_the_entry_points():
    L = _ffi.lib()
    assert L.rayrs_abi_version() == _ffi.ABI_VERSION == 7
    for name in ENTRY_POINTS:
        direct = name.replace("_sky", "_direct")
        assert name in _ffi.SYMBOLS and hasattr(L, name) and getattr(L, name).argtypes == getattr(L, direct).argtypes, name
    for name in HOST_CALLS:
        assert name in _ffi.SYMBOLS and hasattr(L, name), name
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRY_POINTS + HOST_CALLS:
        assert re.search(rf"fn {name}\(", text), name
    assert rayrs_amd.SKY == 0xFFFFFFFF and "SKY" in rayrs_amd.__all__
    assert not any("Sky" in s.__name__ for s in _ffi.ABI_STRUCTS)


# ---- the table, sky_sample and p_env against the reading

def edge_draws(T):
    """(u1, u2) pairs at 0, at 1 - 2^-53, and at values whose product with T (with R_i) is exactly a prefix; how many of
    each kind of exact landing there are."""
    last = F(1.0) - F(2.0) ** -53
    pairs = [(F(0.0), F(0.0)), (last, last), (F(0.0), last), (last, F(0.0)), (F(0.5), F(0.0)), (F(0.5), last)]
    on_row, on_cell = 0, 0
    with np.errstate(all="ignore"):
        for i in range(T.h - 1):
            for u1 in (T.M[i] / T.T, np.nextafter(T.M[i] / T.T, F(0.0)), np.nextafter(T.M[i] / T.T, F(2.0))):
                if 0.0 <= u1 < 1.0:
                    pairs.append((F(u1), F(0.25)))
                    on_row += int(u1 * T.T == T.M[i])
            if not T.R[i] > 0.0:
                continue
            below = T.M[i - 1] if i > 0 else F(0.0)
            u1 = (below + F(0.5) * T.R[i]) / T.T   # (a draw inside row i)
            if not (0.0 <= u1 < 1.0 and T.first_above(T.M, u1 * T.T) == i):
                continue
            for j in range(T.w - 1):
                u2 = T.C[i, j] / T.R[i]
                if 0.0 <= u2 < 1.0:
                    pairs.append((F(u1), F(u2)))
                    on_cell += int(u2 * T.R[i] == T.C[i, j])
    return pairs, on_row, on_cell


@pytest.mark.parametrize("name", list(MAPS))
def test_table_sample_and_density_are_the_readings(name):
    hdri = MAPS[name]
    scene, T = room_scene(hdri), _sky.Table(hdri)
    cells, total = scene.sky_table()
    assert cells.shape == (T.h - 1, T.w - 1) and cells.tobytes() == T.A.tobytes() and F(total).tobytes() == T.T.tobytes()
    assert T.usable()
    if name == "studio":
        assert (T.R == 0.0).any() and (T.A == 0.0).sum() > (T.A > 0.0).sum() and hdri.max() > 3.0   # a zero row, zero cells, the clip
    edges, on_row, on_cell = edge_draws(T)
    print(name, "edge pairs", len(edges), "exactly on a row prefix", on_row, "on a cell prefix", on_cell)
    if name != "two_by_two":   # (one cell: the only prefix is T itself, which no u < 1 reaches)
        assert on_row >= 1 and on_cell >= 1
    rng = np.random.default_rng(7)
    u = np.concatenate([np.array(edges), rng.random((4096 - len(edges), 2))])
    assert u.shape == (4096, 2)
    got = scene.sky_sample(u)
    want = np.array([T.sample(F(a), F(b)) for a, b in u])
    bad = np.flatnonzero((got.view(np.uint64) != want.view(np.uint64)).any(axis=1))
    assert len(bad) == 0, (name, len(bad), [(u[i].tolist(), got[i].tolist(), want[i].tolist()) for i in bad[:3]])
    p = scene.sky_density(got)
    want_p = np.array([T.density(d) for d in got])
    bad = np.flatnonzero(p.view(np.uint64) != want_p.view(np.uint64))
    assert len(bad) == 0, (name, len(bad), [(got[i].tolist(), p[i], want_p[i]) for i in bad[:3]])
    # directions that were not drawn: along the axes (the poles: +inf), into black cells (0), not unit, NaN
    others = np.array([(0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (3.0, -4.0, 0.5),
                       (1e-200, 1e-200, 1e-200), (np.nan, 0.0, 1.0), (0.0, 0.0, 0.0)] + [tuple(v) for v in rng.normal(size=(200, 3))])
    p = scene.sky_density(others)
    want_p = np.array([T.density(d) for d in others])
    nan = np.isnan(want_p)
    assert np.array_equal(np.isnan(p), nan) and p[~nan].tobytes() == want_p[~nan].tobytes(), name   # (a NaN's payload is not the operation's)
    assert (p[0] == np.inf or nan[0]) and (p[1] == np.inf or nan[1]) and nan[-201]


def test_an_all_black_map_has_nothing_to_sample():
    """RAYRS_UNSUPPORTED from every _sky entry point (before RAYRS_NO_DEVICE), and an error from sky_sample and sky_density; the
    table itself can still be read."""
    L = _ffi.lib()
    scene = room_scene(np.zeros((5, 9, 3), dtype=np.float32))
    cells, total = scene.sky_table()
    assert total == 0.0 and not cells.any()
    for call in (lambda: scene.sky_sample(np.zeros((4, 2))), lambda: scene.sky_density(np.ones((4, 3)))):
        with pytest.raises((ValueError, _ffi.RayrsError)):
            call()
    a, b = np.zeros((4, 3)), np.ones((4, 3))
    rad = np.zeros((4, 3))
    P = lambda x: x.ctypes.data
    lamps = np.array([3, 4], dtype=np.uint32)
    for n in (4, 0):
        for lights, nl in ((None, 0), (P(lamps), 2)):
            assert L.rayrs_scene_radiance_sky(scene._h, P(a), P(b), n, 4, 50, 0, 1, 0, 0, lights, nl, P(rad), None) == UNSUPPORTED
            assert L.rayrs_scene_radiance_sky_launch(scene._h, P(a), P(b), n, 4, 50, 0, 1, 0, 0, lights, nl, P(rad), None, None) == UNSUPPORTED
            assert L.rayrs_scene_irradiance_sky(scene._h, P(a), P(b), n, 4, 50, 0, 1e-4, 1, 0, 0, lights, nl, P(rad), None) == UNSUPPORTED
            assert L.rayrs_scene_irradiance_sky_launch(scene._h, P(a), P(b), n, 4, 50, 0, 1e-4, 1, 0, 0, lights, nl, P(rad), None, None) == UNSUPPORTED
            assert L.rayrs_scene_radiance_direct(scene._h, P(a), P(b), n, 4, 50, 0, 1, 0, 0, lights, nl, P(rad), None) == NO_DEVICE
    cam = rayrs_amd.Camera(*scenes.camera_for_resolution(_lit.lit_room()[0], 16, 8))
    img = np.zeros((8, 16, 3))
    assert L.rayrs_render_sky(scene._h, C.byref(cam.desc), 1, 4, 50, 0, 0, None, 0, P(img), None) == UNSUPPORTED
    assert L.rayrs_render_direct(scene._h, C.byref(cam.desc), 1, 4, 50, 0, 0, P(lamps), 2, P(img), None) == NO_DEVICE


@pytest.mark.parametrize("name", ["gradient", "studio"])
def test_the_density_is_the_density_of_the_draws(name):
    """200,000 library draws (the library's draws are the reading's: the test above).  E[1 / p_env] over the draws is the solid
    angle of the set where p_env > 0, the cells that are not black: within 4 standard errors, tests/test_lit.py's margin."""
    hdri = MAPS[name]
    scene, T = room_scene(hdri), _sky.Table(hdri)
    u = np.random.default_rng(11).random((200_000, 2))
    d = scene.sky_sample(u)
    assert np.isfinite(d).all() and np.allclose((d * d).sum(axis=1), 1.0, rtol=0, atol=1e-12)
    p = scene.sky_density(d)
    assert (p > 0.0).all()
    inv = 1.0 / p
    mean, se = inv.mean(), inv.std(ddof=1) / np.sqrt(len(inv))
    want = T.lit_solid_angle()
    print(name, "mean of 1 / p_env", mean, "solid angle of the lit cells", want, "difference / se", (mean - want) / se, "of the sphere", want / (4 * np.pi))
    assert abs(mean - want) <= 4.0 * se, (name, mean, want, se)
    if name == "gradient":
        assert abs(want - 4.0 * np.pi) < 1e-9
    else:
        assert want < 0.5 * 4.0 * np.pi


# ---- Python

def test_sky_in_a_list_reaches_the_sky_entry_points_only_with_direct():
    scene = room_scene(MAPS["studio"])
    a, b = np.zeros((4, 3)), np.ones((4, 3))
    cam = rayrs_amd.Camera(*scenes.camera_for_resolution(_lit.lit_room()[0], 16, 8))
    for f in (scene.radiance, scene.irradiance):
        for lights in ([SKY], [3, SKY, 4], [SKY, SKY, 3], [SKY] * 12):
            with pytest.raises(_ffi.RayrsError) as e:
                f(a, b, lights=lights, direct=True)
            assert e.value.status == NO_DEVICE, lights   # (the _direct call refuses the index: RAYRS_INVALID_ARG)
        with pytest.raises(_ffi.RayrsError) as e:   # nine lamps beside the sky are too many
            f(a, b, lights=[3] * 9 + [SKY], direct=True)
        assert e.value.status == UNSUPPORTED
        with pytest.raises(_ffi.RayrsError) as e:   # without direct: the lit entry point's refusal of the index
            f(a, b, lights=[3, SKY])
        assert e.value.status == INVALID_ARG
    with pytest.raises(_ffi.RayrsError) as e:
        rayrs_amd.render_lit(scene, cam, 2, [SKY], direct=True)
    assert e.value.status == NO_DEVICE
    with pytest.raises(_ffi.RayrsError) as e:
        rayrs_amd.render_lit(scene, cam, 2, [SKY])
    assert e.value.status == INVALID_ARG
    black = room_scene(np.zeros((5, 9, 3), dtype=np.float32))
    with pytest.raises(_ffi.RayrsError) as e:
        black.radiance(a, b, lights=[SKY], direct=True)
    assert e.value.status == UNSUPPORTED
    hdri = procedural.make_studio_hdri(45, 20)
    assert hdri.shape == (20, 45, 3) and hdri.dtype == np.float32 and (hdri[12:] == 0.0).all() and ((hdri != 0.0).any(axis=2).sum() < 45 * 20 // 4)
    assert len({tuple(v) for v in hdri.reshape(-1, 3)}) == 3   # black and the two rectangles


# ---- refusals

scene_names = {}


def host_scene(hdri):
    """tests/test_direct.py's host-only scene: the room, a triangle, and spheres for the material rule."""
    cam, objs, heur, names = _lit.lit_room()
    objs = objs + [Object.triangle((0, 0, 0), (1, 0, 0), (0, 1, 0), Material.NoReflect(), Emission.Dark())]
    tri = len(objs) - 1
    glow = Emission.new(5.0, (1.0, 1.0, 1.0))
    plastic = Material.Plastic((0.7, 0.2, 0.2), (1.0, 1.0, 1.0), 0.2, 1.5)
    extra = [("plastic_lamp", plastic, glow), ("noreflect_lamp", Material.NoReflect(), glow), ("plastic_dark", plastic, Emission.Dark()),
             ("refract_lamp", Material.Refract((0.9, 0.9, 0.9), 1.3), glow), ("glass_lamp", Material.Glass((1, 1, 1), 1.45), glow),
             ("noreflect_dark", Material.NoReflect(), Emission.Dark())]
    for i, (name, mat, em) in enumerate(extra):
        scene_names[name] = len(objs)
        objs.append(Object.sphere(0.1, (3.0, 0.2, -3.0 + 0.5 * i), mat, em))
    return rayrs_amd.Scene(objs, Z_NEAR, Z_FAR, heur, hdri, device=-1), tri


@pytest.mark.parametrize("n", [4, 0])
def test_refusals_on_a_host_only_scene_come_in_the_headers_order(n):
    """DIRECT LIGHTING's refusals in its order (tests/test_direct.py's cases), and after the material rule the empty table: what a
    lit sky accepts (RAYRS_NO_DEVICE) a black sky refuses as RAYRS_UNSUPPORTED, and what is refused earlier is refused the same
    under either."""
    L = _ffi.lib()
    scene, tri = host_scene(MAPS["studio"])
    black, _ = host_scene(np.zeros((5, 9, 3), dtype=np.float32))
    N = scene_names
    a, b = np.zeros((4, 3)), np.ones((4, 3))
    rad, cnt = np.zeros((4, 3)), np.zeros(4, dtype=np.uint32)
    P = lambda x: x.ctypes.data
    good = np.array([3, 4, 5], dtype=np.uint32)

    def call(irr, launch, sc, a_=P(a), b_=P(b), samples=4, bounces=50, chunk=0, fast=0, lights=good, n_lights=None, rad_=P(rad), cnt_=P(cnt),
             no_scene=False):
        lp = None if lights is None else P(lights)
        nl = (0 if lights is None else len(lights)) if n_lights is None else n_lights
        args = (None if no_scene else sc._h, a_, b_, n, samples, bounces, chunk) + ((1e-4,) if irr else ()) + (1, 0, fast, lp, nl, rad_, cnt_)
        name = "rayrs_scene_irradiance_sky" if irr else "rayrs_scene_radiance_sky"
        return getattr(L, name + "_launch")(*args, None) if launch else getattr(L, name)(*args)

    u32 = lambda *v: np.array(v, dtype=np.uint32)
    nine = u32(3, 4, 5, 3, 4, 5, 3, 4, 5)
    for irr in (False, True):
        for launch in (False, True):
            for sc in (scene, black):
                for bad in (dict(no_scene=True), dict(a_=None), dict(b_=None), dict(rad_=None, cnt_=None), dict(samples=0), dict(fast=2),
                            dict(lights=None, n_lights=3), dict(lights=u32(3, 100)), dict(lights=u32(0xffffffff)),
                            dict(lights=u32(N["plastic_lamp"], 100))):
                    assert call(irr, launch, sc, **bad) == INVALID_ARG, (irr, launch, bad)
                    if "samples" not in bad:
                        assert call(irr, launch, sc, bounces=8001, **bad) == INVALID_ARG
                        assert call(irr, launch, sc, samples=1 << 30, **bad) == INVALID_ARG
                for big in (dict(samples=1 << 30), dict(bounces=8001), dict(samples=1 << 20, bounces=2048),
                            dict(samples=(1 << 21) + 1, chunk=1, bounces=1),
                            dict(samples=(1 << 30) - 1, bounces=2, chunk=1 << 12),   # (2^30 - 1) * 5 >= 2^32, where * 2 is not
                            dict(lights=nine), dict(lights=u32(3, tri)), dict(lights=u32(tri)),
                            dict(lights=u32(N["plastic_lamp"])), dict(lights=u32(N["noreflect_lamp"])), dict(lights=u32(N["refract_lamp"])),
                            dict(lights=u32(3, 4, N["plastic_lamp"], 5))):
                    assert call(irr, launch, sc, **big) == UNSUPPORTED, (irr, launch, big)
            for ok in (dict(), dict(fast=1), dict(rad_=None), dict(cnt_=None), dict(bounces=0), dict(lights=None), dict(lights=u32(), n_lights=0),
                       dict(lights=u32(3, 3, 3, 3, 4, 4, 4, 4)), dict(lights=u32(0, 1, 2)), dict(samples=1 << 20, chunk=1, bounces=2047),
                       dict(lights=u32(N["plastic_dark"])), dict(lights=u32(N["noreflect_dark"], 3)), dict(lights=u32(N["glass_lamp"]))):
                assert call(irr, launch, scene, **ok) == NO_DEVICE, (irr, launch, ok)
                assert call(irr, launch, black, **ok) == UNSUPPORTED, (irr, launch, ok)
    # the image form
    cam = rayrs_amd.Camera(*scenes.camera_for_resolution(_lit.lit_room()[0], 16, 8))
    img = np.zeros((8, 16, 3))

    def render(sc, cam_=C.byref(cam.desc), samples=4, bounces=50, fast=0, lights=good, out=P(img), cnt_=None, no_scene=False):
        return L.rayrs_render_sky(None if no_scene else sc._h, cam_, 1, samples, bounces, 0, fast, None if lights is None else P(lights),
                                  0 if lights is None else len(lights), out, cnt_)
    for sc in (scene, black):
        for bad in (dict(no_scene=True), dict(cam_=None), dict(out=None), dict(samples=0), dict(fast=2), dict(lights=u32(100)),
                    dict(lights=u32(0xffffffff))):
            assert render(sc, **bad) == INVALID_ARG, bad
            assert render(sc, bounces=8001, **bad) == INVALID_ARG, bad
        for big in (dict(bounces=8001), dict(lights=nine), dict(lights=u32(tri)), dict(lights=u32(N["plastic_lamp"])),
                    dict(lights=u32(N["noreflect_lamp"])), dict(samples=1 << 20, bounces=2048)):
            assert render(sc, **big) == UNSUPPORTED, big
    for ok in (dict(), dict(lights=None), dict(fast=1), dict(lights=u32(N["plastic_dark"])), dict(samples=1 << 20, bounces=2047)):
        assert render(scene, **ok) == NO_DEVICE, ok
        assert render(black, **ok) == UNSUPPORTED, ok


# ---- kernel resources: what the direct kernels are held to (tests/test_direct.py)
VGPR_BOUND = 256


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_the_sky_kernels_use_no_scratch_and_keep_two_waves_per_simd(tmp_path):
    res = kernel_resources(compile_asm("radiance_sky.hip", tmp_path))
    path = {n: r for n, r in res.items() if "radiance_sky_kernel" in n}
    resolve = {n: r for n, r in res.items() if "radiance_sky_resolve_kernel" in n}
    assert len(path) == 12 and len(resolve) == 1 and len(res) == 13   # COMPACT x EXACT x the three starts; the resolve
    for name, (vgpr, scratch, lds) in res.items():
        print(name, vgpr, scratch, lds)
        assert vgpr <= VGPR_BOUND and scratch == 0 and lds == 0, (name, vgpr, scratch, lds)   # (the stacks are dynamic LDS)


# ---- unbiased

def test_sky_irradiance_has_the_unlit_mean():
    """tests/test_direct.py's room, points, sample counts, seeds and margin, under the studio map: the reading's means with the
    lamps and the sky, and with the sky alone, agree with the unlit mean within 4 combined standard errors in every channel.  The
    per-channel variance ratios over unlit (and direct lighting's, lamps only) are printed, not asserted on."""
    hdri = MAPS["studio"]
    cam, objs, heur, names = _lit.lit_room()
    R = _sky.Reading(objs, Z_NEAR, Z_FAR, heur, hdri)
    D = _direct.Reading(objs, Z_NEAR, Z_FAR, heur, hdri, osc=R.osc)
    points = np.array([(0.0, 0.0, 0.0), (1.5, 0.0, -1.5), (-3.0, 0.0, 3.0)])
    normals = np.tile((0.0, 1.0, 0.0), (len(points), 1))
    lamps = [names["sphere_lamp"], names["rect_lamp"]]
    assert lamps == rayrs_amd.emitters(objs)
    s_sky, s_unlit = 2000, 8000
    both, bq = _sky.irradiance_paths(R, points, normals, s_sky, 1e-4, 50, 11, lamps)
    alone, aq = _sky.irradiance_paths(R, points, normals, s_sky, 1e-4, 50, 13, [])
    direct, _ = _direct.irradiance_paths(D, points, normals, s_sky, 1e-4, 50, 11, lamps)
    unlit, uq = _direct.irradiance_paths(D, points, normals, s_unlit, 1e-4, 50, 12, [])
    assert np.isfinite(both).all() and np.isfinite(alone).all() and np.isfinite(unlit).all()
    for i in range(len(points)):
        mu, vu = unlit[i].mean(axis=0), unlit[i].var(axis=0, ddof=1)
        for what, x, q in (("lamps + sky", both, bq), ("sky alone", alone, aq)):
            m, v = x[i].mean(axis=0), x[i].var(axis=0, ddof=1)
            se = np.sqrt(v / s_sky + vu / s_unlit)
            print("point", points[i].tolist(), what, m, "unlit", mu, "difference / se", (m - mu) / se, "variance / unlit", v / vu,
                  "direct / unlit", direct[i].var(axis=0, ddof=1) / vu, "queries per path", q[i].mean(), "unlit", uq[i].mean())
            assert (np.abs(m - mu) <= 4.0 * se).all(), (i, what, m, mu, se)


# ---- every branch

TALLY_SEED = 2
TALLY_Z_FAR = 6.5


def test_the_rooms_paths_take_every_branch():
    """A 24 x 16 x 3 image of the room under the studio map, lamps, a portal and the sky.  A ray aimed at a lamp's own point
    meets that lamp or something in front of it, never nothing: it can miss only through the z window.  So the camera's primary
    directions are made about two units long (their hits lie at t < 5.6) and z_far is 6.5 -- a shadow ray from the near floor to
    the rectangle lamp is longer than that.  The seed is chosen so that this one image shows every branch."""
    cam, objs, heur, names = _lit.lit_room()
    R = _sky.Reading(objs, Z_NEAR, TALLY_Z_FAR, heur, MAPS["studio"])
    ocam = _oracle.OracleCamera(*(cam[:4] + (24 / 25.4 + 1e-9, 16 / 25.4 + 1e-9, 10)))
    assert (ocam.x_pixels(), ocam.y_pixels()) == (24, 16)
    lights = [names["sphere_lamp"], names["rect_lamp"], names["dark_sphere"]]
    tally = _sky.new_tally()
    values, queries = _sky.image_paths(R, ocam, 3, 50, TALLY_SEED, lights, tally=tally)
    print(tally, "queries per path", queries.mean())
    assert np.isfinite(values).all()
    assert tally["sky_credited"] >= 10      # the sky chosen and credited
    assert tally["sky_blocked"] >= 5        # the sky chosen and blocked
    assert tally["sky_skipped_ndl"] >= 10   # the sky chosen and skipped for ndl_s <= 0
    assert tally["sky_met_lamp"] >= 1       # a sky-aimed shadow ray that meets a listed lamp
    assert tally["lamp_missed"] >= 1        # a lamp-aimed shadow ray that misses and is credited the background
    assert tally["miss_weighted"] >= 10     # a miss of the path's own ray with w < 1
    assert tally["miss_unweighted"] >= 10   # ... and with w = 1: a first ray, or after a specular bounce
    assert tally["plastic_diffuse"] >= 1 and tally["plastic_specular"] >= 1
    assert tally["lamp_credited"] >= 100 and tally["lamp_blocked"] >= 1
    assert (queries <= 2 * 50 + 1).all()
