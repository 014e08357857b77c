"""The film's noise plane and the variance-guided a-trous filter (include/rayrs_hip.h NOISE PLANE, GUIDED FILTER) without a
GPU: the boundary's declarations and defining lines, every refusal that is decided before the device is touched, the
soundness of the plain-Python reference the GPU tests compare against (_guided.py), and the new kernels' resources from
the compiled ISA."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _features as F
import _film
import _film_adaptive as A
import _guided as G
import rayrs_amd
from rayrs_amd import _ffi
from test_features import HIPCC, ROOT, compile_asm, kernel_resources

NEW_SYMBOLS = ["rayrs_film_noise", "rayrs_film_denoise_guided", "rayrs_image_denoise_guided"]
INF = float("inf")


def header():
    return open(os.path.join(ROOT, "include", "rayrs_hip.h")).read()


# ------------------------------------------------------------------------------------------------------ the boundary

def test_the_header_declares_the_entry_points_with_their_defining_lines():
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\bint {name}\s*\(", code), name
    assert re.search(r"#define RAYRS_GUIDED_EPS 0x1p-33\b", code)
    text = re.sub(r"\s*\n \*\s*", " ", header())
    assert "v = d / (((m*m)*(m-1.0)) * ((double)c*(double)c))" in text
    assert "e = ((dn*kn + da*ka) + dz*kz) + (dl*dl)*r_p" in text
    assert "vs += (ww == 0) ? +0 : v_q*ww" in text
    assert "RAYRS_GUIDED_EPS = 2^-33" in text
    assert "g[0] = 1/2, g[1] = 1/4" in text
    assert "r_p = (gw == 0) ? +0 : kv / (gs/gw + RAYRS_GUIDED_EPS)" in text
    assert "no variance-guided weight" not in text
    assert G.EPS == float.fromhex("0x1p-33")


def test_the_library_exports_the_entry_points():
    L = _ffi.lib()
    for name in NEW_SYMBOLS:
        assert name in _ffi.SYMBOLS and hasattr(L, name), name
    assert hasattr(rayrs_amd, "denoise_guided") and "denoise_guided" in rayrs_amd.__all__
    assert hasattr(rayrs_amd.Film, "noise") and hasattr(rayrs_amd.Film, "denoised_guided")
    assert rayrs_amd.api.SIGMA_LUMINANCE == 4.0 and rayrs_amd.api._k(rayrs_amd.api.SIGMA_LUMINANCE) == 1.0 / 16.0
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"fn {name}\(", text), name


def test_the_abi_version_and_the_layout_table_are_unchanged():
    L = _ffi.lib()
    assert L.rayrs_abi_version() == _ffi.ABI_VERSION == 7
    want = [7]
    for st in _ffi.ABI_STRUCTS:
        want += [C.sizeof(st), len(st._fields_)] + [getattr(st, name).offset for name, _ in st._fields_]
    n = L.rayrs_abi_layout(None, 0)
    table = (C.c_uint32 * n)()
    assert L.rayrs_abi_layout(table, n) == n
    assert list(table) == want
    assert len(_ffi.ABI_STRUCTS) == 9 and _ffi.ABI_STRUCTS[-2:] == [_ffi.FilmParams, _ffi.FilmStatus]


# ------------------------------------------------------------------------------------------------------ refusals

def test_guided_refusals_before_the_device_is_touched():
    """device = -1 stands for "no device": every parameter refusal must come before RAYRS_NO_DEVICE."""
    L = _ffi.lib()
    color, var, out, out_var = np.zeros((4, 4, 3)), np.zeros((4, 4)), np.zeros((4, 4, 3)), np.zeros((4, 4))

    def call(levels=5, k=(1.0, 1.0, 1.0, 1.0), w=4, h=4, c=color, v=var, o=out, ov=out_var):
        ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        return L.rayrs_image_denoise_guided(-1, w, h, ptr(c), ptr(v), None, None, None, levels, *k, ptr(o), ptr(ov))

    assert call(levels=0) == -1 and call(levels=17) == -1
    for i in range(4):
        for bad in (-1.0, float("nan"), INF, -0.5):
            k = [1.0] * 4
            k[i] = bad
            assert call(k=tuple(k)) == -1, (i, bad)
    assert call(c=None) == -1 and call(v=None) == -1 and call(o=None) == -1 and call(w=0) == -1 and call(h=0) == -1
    assert call(w=70000, h=1) == -5 and call(w=1, h=65536) == -5
    assert call(w=70000, h=1, levels=0) == -1             # a parameter refusal comes first
    assert call() == -4 and call(ov=None) == -4 and call(levels=1, k=(0.0, 0.0, 0.0, 0.0)) == -4 and call(levels=16) == -4
    with pytest.raises(_ffi.RayrsError) as e:
        rayrs_amd.denoise_guided(color, var, device=-1)
    assert e.value.status == -4
    with pytest.raises(ValueError):
        rayrs_amd.denoise_guided(color, None, device=-1)
    with pytest.raises(ValueError):
        rayrs_amd.denoise_guided(color, np.zeros((4, 5)), device=-1)


def test_film_refusals_on_a_host_only_scene():
    L = _ffi.lib()
    buf = np.zeros(16)
    assert L.rayrs_film_noise(None, buf.ctypes.data) == -1
    assert L.rayrs_film_denoise_guided(None, 16, 5, 1.0, 1.0, 1.0, 1.0, 1, buf.ctypes.data, None) == -1
    # a host-only scene makes no film, so there is nothing the film calls could be handed
    cam_args, objs, heur, env = _film.sphere_desc()
    scene, cam = rayrs_amd.Scene(objs, 1e-6, 1e6, heur, env, device=-1), rayrs_amd.Camera(*cam_args)
    with pytest.raises(_ffi.RayrsError) as e:
        rayrs_amd.Film(scene, cam)
    assert e.value.status == -4


# ------------------------------------------------------------------------------------------------------ the reference

K = (4.0, 25.0, 0.3)   # kn, ka, kz


def test_an_all_infinite_variance_reproduces_the_feature_guided_filter():
    w, h = 13, 9
    color, normal, albedo, depth = F.random_case(11, w, h)
    var = np.full((h, w), INF)
    want = F.atrous_levels(color, normal, albedo, depth, 4, *K, 0.0)
    got = G.guided_levels(color, var, normal, albedo, depth, 4, *K, 1.0 / 16.0)
    for level, (a, (b, v)) in enumerate(zip(want, got)):
        assert F.same_bits(a, b), level
        # the variance stays +inf wherever the pixel was filtered, and passes through elsewhere
        assert ((v == INF) | ~np.isfinite(color).all(axis=2)).all() and not np.isnan(v).any()


def test_a_flat_frame_scales_an_interior_variance_by_the_squared_weights():
    flat, var = np.full((9, 9, 3), 0.25), np.full((9, 9), 0.5)
    color, v = G.guided(flat, var, None, None, None, 1, 0.0, 0.0, 0.0, 1.0 / 16.0)
    factor = (70.0 / 256.0) ** 2
    assert factor == 0.07476806640625
    assert abs(v[4, 4] / 0.5 - factor) <= 1e-12 * factor
    assert np.abs(color - 0.25).max() < 1e-15
    assert v[0, 0] > v[4, 4]      # fewer taps at a corner: less averaging


def test_awkward_variances_and_colours_make_no_new_nan_and_pass_through():
    w, h = 33, 17
    color, normal, albedo, depth = F.random_case(3, w, h)
    var = G.random_variance(4, w, h)
    assert np.isnan(var).sum() == 1 and (var < 0).sum() == 1 and (var == INF).any() and (var == 0).any()
    bad_c = ~np.isfinite(color).all(axis=2)
    nan_in = np.isnan(color).any(axis=2)
    for level, (c, v) in enumerate(G.guided_levels(color, var, normal, albedo, depth, 4, *K, 1.0 / 16.0)):
        assert F.same_bits(c[bad_c], color[bad_c]) and F.same_bits(v[bad_c], var[bad_c]), level   # passed through
        assert (np.isnan(c).any(axis=2) == nan_in).all(), level                                   # no new NaN in the colour
        # the variance: a NaN only where the input held one and the pixel could not be filtered
        assert (np.isnan(v) <= np.isnan(var)).all(), level
        assert (v[~np.isnan(v) & ~bad_c & np.isfinite(normal).all(axis=2)] >= 0.0).all(), level
    # a pixel whose own variance is NaN or negative is still filtered from its neighbours
    y, x = np.argwhere((var < 0) | np.isnan(var))[0]
    if not bad_c[y, x] and np.isfinite(normal[y, x]).all():
        c1, v1 = G.guided(color, var, normal, albedo, depth, 1, *K, 1.0 / 16.0)
        assert v1[y, x] >= 0.0 and not F.same_bits(c1[y, x], color[y, x])


@pytest.mark.parametrize("name", ["sphere"])
def test_the_noise_plane_is_infinite_exactly_below_two_chunks(name):
    rgb, it = A.named_traces(name, 8, _film.W, _film.H)
    rep = A.Replay(rgb, it)
    rep.nt[:] = 8
    rep.nt[0, :] = 4          # M = 1 in the first row of tiles
    rep.nt[1, 1] = 0          # and an empty tile
    s1, s2 = rep.sums()
    assert np.isfinite(s1).all() and np.isfinite(s2).all()
    plane = G.noise_plane(s1, s2, rep.nt, rep.c)
    m = np.repeat(np.repeat(rep.nt // rep.c, 8, axis=0), 8, axis=1)[:rep.h, :rep.w]
    assert ((plane == INF) == (m < 2)).all() and (m < 2).any() and (m >= 2).any()
    assert not np.isnan(plane).any() and (plane >= 0.0).all() and (plane[m >= 2] > 0.0).any()
    # the plane is the sample variance of the chunk sums over M and c^2
    y, x = np.argwhere((m >= 2) & (plane > 0))[0]
    sums = [rgb[y, x, lo:lo + 4].sum(axis=0).sum() for lo in (0, 4)]
    assert abs(plane[y, x] - np.var(sums, ddof=1) / 2 / 16) <= 1e-9 * plane[y, x]
    # outside a share: +0
    share = np.zeros_like(rep.share)
    share[::2] = True
    part = G.noise_plane(s1, s2, rep.nt, rep.c, share)
    outside = ~np.repeat(np.repeat(share, 8, axis=0), 8, axis=1)[:rep.h, :rep.w]
    assert (part[outside] == 0.0).all() and F.same_bits(part[~outside], plane[~outside])
    # non-finite sums select +inf, and a difference that is not positive +0
    assert G.noise_value(INF, 1.0, 8, 4) == INF and G.noise_value(1.0, float("nan"), 8, 4) == INF
    assert G.noise_value(1e200, 1e200, 8, 4) == INF          # d overflows
    assert G.noise_value(2.0, 2.0, 8, 4) == 0.0 and G.noise_value(3.0, 2.0, 8, 4) == 0.0
    assert G.noise_value(1.0, 1.0, 7, 4) == INF and G.noise_value(1.0, 1.0, 8, 4) == 1.0 / (4.0 * 16.0)


# ------------------------------------------------------------------------------------------------------ the kernels

needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@needs_hipcc
def test_the_guided_kernels_keep_their_occupancy_class(tmp_path):
    """the guided a-trous kernel 6 waves per SIMD (at most 80 registers; it compiles to 79), the noise-plane
    and pack kernels 8 (at most 64), and beside them in the unit the plain a-trous kernel 7 (at most 72); no scratch and no LDS
    in any of them."""
    res = kernel_resources(compile_asm("denoise.hip", tmp_path))
    assert len(res) == 4
    # ("13atrous_kernel": the mangled name's length prefix tells atrous_kernel from guided_atrous_kernel)
    bounds = {"film_noise_kernel": 64, "guided_pack_kernel": 64, "guided_atrous_kernel": 80, "13atrous_kernel": 72}
    for key, bound in bounds.items():
        (name, (vgpr, scratch, lds)), = [(n, r) for n, r in res.items() if key in n]
        assert vgpr <= bound and scratch == 0 and lds == 0, (name, vgpr, scratch, lds)
