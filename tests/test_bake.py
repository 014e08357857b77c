"""The bake (include/rayrs_hip.h BAKE) without a GPU: the header states the contract and the binding declares the entry points,
every refusal of a creation that is decided before the device is touched comes in the header's order on a host-only scene, Bake
refuses its arguments, the calls refuse a NULL bake, and the per-point replay the GPU tests hold the library to (tests/_bake.py) is
a second, independent fold's answer on a handful of points.  (A bake exists on a device scene only, so what rayrs_bake_state_set
refuses of a foreign image is tests/test_gpu_bake.py's.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _bake as B
import _lit
import rayrs_amd
from rayrs_amd import SKY, _ffi
from test_sky import MAPS, host_scene, room_scene, scene_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["rayrs_bake_create", "rayrs_bake_destroy", "rayrs_bake_render", "rayrs_bake_render_adaptive", "rayrs_bake_read",
                "rayrs_bake_point_samples", "rayrs_bake_noise", "rayrs_bake_status_get", "rayrs_bake_state_bytes", "rayrs_bake_state_get",
                "rayrs_bake_state_set"]
INVALID_ARG, NO_DEVICE, UNSUPPORTED = -1, -4, -5


def header():
    return open(os.path.join(ROOT, "include", "rayrs_hip.h")).read()


def test_the_header_states_the_contract_and_the_binding_declares_the_entry_points():
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(rf"\b{name}\s*\(", code), name
        assert name in _ffi.SYMBOLS and hasattr(_ffi.lib(), name), name
    text = re.sub(r"\s+", " ", re.sub(r"\s*\n \*\s*", " ", header()))
    assert text.index("DIRECT-LIT FILMS.") < text.index("BAKE.") < text.index("The boundary's version")
    for words in ("THE CONTRACT PER POINT", "index_base = index_base + i", "the read is sum * (1.0 / N_i)", "(largest N_i) + n < 2^30",
                  "ceil(n / c) > 65536", "takes point i iff N_i + n <= max_point_samples", "a non-finite point is never taken",
                  "in ascending index order", "n >= 2^32. Then RAYRS_NO_DEVICE", "The points, the scene and the list are NOT recorded"):
        assert words in text, words
    assert int(re.search(r"#define RAYRS_ABI_VERSION (\d+)", header()).group(1)) == _ffi.lib().rayrs_abi_version() == 7
    # the mirrors have the C layout of the header's structs (all fields 4 or 8 bytes wide and naturally aligned)
    assert C.sizeof(_ffi.BakeParams) == 48 and _ffi.BakeParams.seed.offset == 16 and _ffi.BakeParams.sky.offset == 40
    assert C.sizeof(_ffi.BakePass) == 48 and C.sizeof(_ffi.BakeStatus) == 56
    for st, cname in ((_ffi.BakeParams, "rayrs_bake_params"), (_ffi.BakePass, "rayrs_bake_pass"), (_ffi.BakeStatus, "rayrs_bake_status")):
        body = re.search(r"typedef struct \{([^}]*)\} " + cname + ";", code).group(1)
        names = [n.strip() for decl in re.findall(r"(?:uint32_t|uint64_t|double)\s+([^;]+);", body) for n in decl.split(",")]
        assert names == [n for n, _ in st._fields_], cname


def test_bake_refuses_its_arguments_without_a_device():
    scene = room_scene(MAPS["studio"])
    p, n = np.zeros((4, 3)), np.tile((0.0, 1.0, 0.0), (4, 1))
    for bad in (dict(direct=True), dict(lights=[3, 4]), dict(lights=[]), dict(lights=[-1], direct=True), dict(kind="pixels")):
        with pytest.raises(ValueError):
            rayrs_amd.Bake(scene, p, n, **bad)
    with pytest.raises(ValueError):
        rayrs_amd.Bake(scene, p, n[:3])
    with pytest.raises(ValueError):
        rayrs_amd.Bake(scene, np.zeros(3), np.zeros(3))
    # what reaches the library is refused there: the scene has no device
    for kw in (dict(), dict(kind="radiance"), dict(lights=[3, 4], direct=True), dict(lights=[], direct=True), dict(lights=[SKY], direct=True),
               dict(lights=[3, SKY, 4], direct=True), dict(fast_traversal=True), dict(max_bounces=0)):
        with pytest.raises(_ffi.RayrsError) as e:
            rayrs_amd.Bake(scene, p, n, **kw)
        assert e.value.status == NO_DEVICE, kw
    with pytest.raises(_ffi.RayrsError) as e:
        rayrs_amd.Bake(scene, p, n, lights=[100], direct=True)
    assert e.value.status == INVALID_ARG
    black = room_scene(np.zeros((5, 9, 3), dtype=np.float32))
    with pytest.raises(_ffi.RayrsError) as e:
        rayrs_amd.Bake(black, p, n, lights=[SKY], direct=True)
    assert e.value.status == UNSUPPORTED
    with pytest.raises(_ffi.RayrsError) as e:
        rayrs_amd.Bake(black, p, n, lights=[3], direct=True)
    assert e.value.status == NO_DEVICE


def test_refusals_at_creation_come_in_the_headers_order():
    """On the host-only room with a triangle and the material rule's spheres (tests/test_sky.py host_scene), under a lit and under
    a black sky: each condition alone, and beside one of a later group."""
    L = _ffi.lib()
    scene, tri = host_scene(MAPS["studio"])
    black, _ = host_scene(np.zeros((5, 9, 3), dtype=np.float32))
    N = scene_names
    u32 = lambda *v: np.array(v, dtype=np.uint32)
    good, nine = u32(3, 4, 5), u32(3, 4, 5, 3, 4, 5, 3, 4, 5)
    pts = np.zeros((4, 3))

    def call(sky, sc, lights=good, n_lights=None, n=4, no_scene=False, no_a=False, no_b=False, no_params=False, no_out=False, kind=0,
             chunk=2, bounces=50, fast=0, pad=0, sky_word=None):
        p = _ffi.BakeParams()
        p.kind, p.sample_chunk, p.max_bounces, p.fast_traversal, p.seed, p.pad = kind, chunk, bounces, fast, 1, pad
        p.sky = (1 if sky else 0) if sky_word is None else sky_word
        h = C.c_void_p()
        nl = (0 if lights is None else len(lights)) if n_lights is None else n_lights
        st = L.rayrs_bake_create(None if no_scene else sc._h, None if no_a else pts.ctypes.data, None if no_b else pts.ctypes.data, n,
                                 None if no_params else C.byref(p), None if lights is None or len(lights) == 0 else lights.ctypes.data, nl,
                                 None if no_out else C.byref(h))
        assert not h.value
        return st

    invalid = (dict(no_scene=True), dict(no_a=True), dict(no_b=True), dict(no_params=True), dict(no_out=True), dict(fast=2), dict(pad=1),
               dict(kind=2), dict(sky_word=2), dict(lights=None, n_lights=3), dict(lights=u32(3, 100)), dict(lights=u32(0xffffffff)),
               dict(lights=u32(N["plastic_lamp"], 100)))
    unsupported = (dict(bounces=8001), dict(chunk=1 << 30), dict(lights=nine), dict(lights=u32(3, tri)), dict(lights=u32(tri)),
                   dict(lights=u32(N["plastic_lamp"])), dict(lights=u32(N["noreflect_lamp"])), dict(lights=u32(N["refract_lamp"])),
                   dict(lights=u32(3, 4, N["plastic_lamp"], 5)),
                   dict(chunk=1 << 20, bounces=2048),   # 2^20 * 4097 >= 2^32
                   dict(n=1 << 32), dict(n=(1 << 32) + 5))
    later = (dict(bounces=8001), dict(chunk=1 << 30), dict(n=1 << 32))
    ok = (dict(), dict(fast=1), dict(kind=1), dict(n=0), dict(n=(1 << 32) - 1), dict(lights=u32(3, 3, 3, 3, 4, 4, 4, 4)), dict(lights=u32(0, 1, 2)),
          dict(lights=u32(N["plastic_dark"])), dict(lights=u32(N["noreflect_dark"], 3)), dict(lights=u32(N["glass_lamp"])),
          dict(chunk=1 << 20, bounces=2047), dict(chunk=0), dict(bounces=0))
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
            # the empty table is the sky bake's refusal alone, after the material rule and before the device
            assert call(sky, black, **good_call) == (UNSUPPORTED if sky else NO_DEVICE), (sky, good_call)
    # the unlit bake (no list, no sky) counts max_bounces queries a sample, the others 2 * max_bounces + 1
    none = dict(lights=None)
    assert call(False, scene, chunk=1 << 20, bounces=2048, **none) == NO_DEVICE        # 2^20 * 2048 = 2^31
    assert call(False, scene, chunk=1 << 20, bounces=4095, **none) == NO_DEVICE
    assert call(False, scene, chunk=1 << 20, bounces=4096, **none) == UNSUPPORTED      # 2^32
    assert call(True, scene, chunk=1 << 20, bounces=2048, **none) == UNSUPPORTED       # (the sky alone is no unlit bake)
    assert call(False, scene, chunk=1 << 20, bounces=4096, kind=2, **none) == INVALID_ARG


def test_the_calls_refuse_a_missing_bake():
    L = _ffi.lib()
    buf = np.zeros(256, dtype=np.uint8)
    st, ps, act = _ffi.BakeStatus(), _ffi.BakePass(), C.c_uint64(7)
    assert L.rayrs_bake_render(None, 2, C.byref(ps)) == INVALID_ARG
    assert L.rayrs_bake_render_adaptive(None, 2, 0.1, 0, C.byref(act), C.byref(ps)) == INVALID_ARG
    assert L.rayrs_bake_read(None, buf.ctypes.data, None) == INVALID_ARG
    assert L.rayrs_bake_point_samples(None, buf.ctypes.data) == INVALID_ARG
    assert L.rayrs_bake_noise(None, buf.ctypes.data) == INVALID_ARG
    assert L.rayrs_bake_status_get(None, 0.1, C.byref(st)) == INVALID_ARG
    assert L.rayrs_bake_state_bytes(None) == 0
    assert L.rayrs_bake_state_get(None, buf.ctypes.data, 256) == INVALID_ARG
    assert L.rayrs_bake_state_set(None, buf.ctypes.data, 256) == INVALID_ARG
    L.rayrs_bake_destroy(None)
    assert act.value == 7


# ---- the GPU tests' replay is a second fold's answer

def fold(values, c, n):
    """One point, scalar by scalar: (value (3,), S1, S2, M) after n samples in chunks of c, by the header's words."""
    total, s1, s2, m = None, 0.0, 0.0, 0
    with np.errstate(all="ignore"):
        for lo in range(0, n, c):
            hi = min(lo + c, n)
            cs = [np.float64(0.0)] * 3
            for s in range(lo, hi):
                cs = [cs[k] + values[s][k] for k in range(3)]
            total = cs if total is None else [total[k] + cs[k] for k in range(3)]
            if hi - lo == c:
                y = (cs[0] + cs[1]) + cs[2]
                s1, s2 = (y, y * y) if m == 0 else (s1 + y, s2 + y * y)
                m += 1
        inv = np.float64(1.0) / np.float64(n)
        return np.array([t * inv for t in total]), s1, s2, m


def unconverged(s1, s2, m, tau):
    if not (np.isfinite(s1) and np.isfinite(s2)):
        return False
    with np.errstate(all="ignore"):
        mf = np.float64(m)
        s11 = s1 * s1
        return not (m >= 2 and mf * s2 - s11 <= ((np.float64(tau) * np.float64(tau)) * s11) * (mf - np.float64(1.0)))


HANDFUL = (0, 63, 64, 65, 129)


@pytest.mark.parametrize("strategy", B.STRATEGIES)
def test_the_replay_is_a_second_folds_answer_on_a_handful_of_points(strategy):
    values, q = B.paths("room", strategy, "irradiance")
    assert values.shape == (B.N_POINTS, B.N_MAX, 3) and q.shape == (B.N_POINTS, B.N_MAX) and np.isfinite(values).all()
    tau, cap = 0.3, 8
    rep = B.Replay(values, q)
    ni = {i: 0 for i in HANDFUL}
    for kind in ("adaptive", "uniform", "adaptive", "adaptive"):
        taken = {}
        for i in HANDFUL:   # the second fold decides first, from the counts before the pass
            s1, s2, m = fold(values[i], B.C, ni[i])[1:] if ni[i] else (0.0, 0.0, 0)
            taken[i] = kind == "uniform" or (ni[i] + 2 <= cap and unconverged(s1, s2, m, tau))
        got = rep.adaptive_pass(2, tau, cap) if kind == "adaptive" else rep.uniform_pass(2)
        for i in HANDFUL:
            assert bool(got["active"][i]) == taken[i], (kind, i)
            ni[i] += 2 if taken[i] else 0
            assert int(got["ni"][i]) == ni[i]
            value, s1, s2, m = fold(values[i], B.C, ni[i])
            assert np.array_equal(got["values"][i].view(np.uint64), value.view(np.uint64)), (kind, i)
            assert int(got["queries"][i]) == int(q[i, :ni[i]].sum())
            assert bool(rep.masks(tau)[0][i]) == unconverged(s1, s2, m, tau)
    # the short last chunk is in the value and not in the statistics; the noise is NOISE PLANE's formula
    rep = B.Replay(values, q)
    for n in (2, 4, 3):
        rep.uniform_pass(n)
    assert rep.closed
    noise = rep.noise()
    for i in HANDFUL:
        value, s1, s2, m = fold(values[i], B.C, 9)
        assert m == 4 and np.array_equal(rep.values()[i].view(np.uint64), value.view(np.uint64))
        d = 4.0 * s2 - s1 * s1
        assert noise[i] == (d / (((4.0 * 4.0) * 3.0) * (2.0 * 2.0)) if d > 0 else 0.0)
    assert (B.Replay(values, q).noise() == np.inf).all()


def test_the_points_are_hits_and_their_normals_face_their_rays():
    for name in ("room", "mesh1_light"):
        o, d, p, nrm = B.geometry(name)
        assert o.shape == d.shape == p.shape == nrm.shape == (B.N_POINTS, 3)
        assert ((nrm * d).sum(axis=1) < 0).all() and np.isfinite(p).all()
        assert len(np.unique(p, axis=0)) == B.N_POINTS
