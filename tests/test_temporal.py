"""Temporal accumulation (include/rayrs_hip.h TEMPORAL ACCUMULATION) without a GPU: the boundary's declarations and defining
lines, every refusal that is decided before the device is touched, rayrs_camera_orbit against the oracle's sine and cosine,
the soundness of the plain-Python reading the GPU tests compare against (_temporal.py) -- its projection against the
oracle's camera, its properties, and that the GPU test's case list takes every branch of it -- and the reprojection
kernel's resources from the compiled ISA."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import _features as F
import _film
import _oracle
import _temporal as T
import rayrs_amd
from rayrs_amd import _ffi
from test_features import HIPCC, ROOT, compile_asm, kernel_resources
from test_numeric import path_key

NEW_SYMBOLS = ["rayrs_history_create", "rayrs_history_destroy", "rayrs_history_reset", "rayrs_history_push_image",
               "rayrs_history_push_film", "rayrs_history_push_times", "rayrs_history_read", "rayrs_history_denoise_guided",
               "rayrs_camera_orbit"]
INF = float("inf")


def header():
    return open(os.path.join(ROOT, "include", "rayrs_hip.h")).read()


# ------------------------------------------------------------------------------------------------------ the boundary

def test_the_header_declares_the_entry_points_with_their_defining_lines():
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b(int|void) {name}\s*\(", code), name
    text = re.sub(r" +", " ", re.sub(r"\s*\n \*\s*", " ", header()))
    for line in ("x = ((double)(W - col) + 0.5) / (double)ppc - width/2.",
                 "y = ((double)(H - r) + 0.5) / (double)ppc - height/2.",
                 "d = (z_cam + x*e_x) + y*e_y",
                 "T = z_p / k_p, P = origin_A + d*T, u = P - origin_B",
                 "s = dot(u, z'), zz = dot(z', z')",
                 "xp = (dot(u,e_x')*zz)/s, yp = (dot(u,e_y')*zz)/s",
                 "fx = ((double)W' + 0.5) - (xp + width'/2.)*(double)ppc'",
                 "fy = ((double)H' + 0.5) - (yp + height'/2.)*(double)ppc'",
                 "fx >= -1 && fx < W' && fy >= -1 && fy < H'",
                 "b = (i ? ax : 1-ax) * (j ? ay : 1-ay)",
                 "dt*dt <= tz2*(tp*tp)",
                 "((n_p.x-n'_q.x)^2 + (n_p.y-n'_q.y)^2) + (n_p.z-n'_q.z)^2 <= tn2",
                 "M = (M0 < max_weight) ? M0 : max_weight",
                 "vp = (V*M0)/wc_p", "V = (vp*wc_p)/M0",
                 "alpha = wc_p/(wc_p + M), beta = 1 - alpha",
                 "tb = (beta*beta == 0) ? +0 : V*(beta*beta)",
                 "out weight = M + wc_p",
                 "out = lookat + ((v*c + x*s) + k*g)",
                 "KNOWN LIMIT"):
        assert line in text, line
    assert "nothing temporal (that is TEMPORAL ACCUMULATION below)" in text


def test_the_library_exports_the_entry_points():
    L = _ffi.lib()
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_SYMBOLS:
        assert name in _ffi.SYMBOLS and hasattr(L, name), name
        assert re.search(rf"fn {name}\(", text), name
    for name in ("History", "orbit", "render_sequence"):
        assert hasattr(rayrs_amd, name) and name in rayrs_amd.__all__, name
    for method in ("push", "push_image", "image", "variance", "weight", "denoised_guided", "reset"):
        assert hasattr(rayrs_amd.History, method), method


def test_the_abi_version_and_the_layout_table_are_unchanged():
    L = _ffi.lib()
    assert L.rayrs_abi_version() == _ffi.ABI_VERSION == 7
    assert re.search(r"#define RAYRS_ABI_VERSION 7\b", header())
    want = [7]
    for st in _ffi.ABI_STRUCTS:
        want += [C.sizeof(st), len(st._fields_)] + [getattr(st, name).offset for name, _ in st._fields_]
    n = L.rayrs_abi_layout(None, 0)
    table = (C.c_uint32 * n)()
    assert L.rayrs_abi_layout(table, n) == n
    assert list(table) == want
    assert len(_ffi.ABI_STRUCTS) == 9


# ------------------------------------------------------------------------------------------------------ refusals

def new_history(device=-1):
    h = C.c_void_p()
    assert _ffi.lib().rayrs_history_create(device, C.byref(h)) == 0 and h.value
    return h


def test_refusals_before_the_device_is_touched():
    """device = -1 stands for "no device": every parameter refusal must come before RAYRS_NO_DEVICE."""
    L = _ffi.lib()
    assert L.rayrs_history_create(-1, None) == -1
    h = new_history()
    cam = rayrs_amd.Camera((0, 1, 5), (0, 1, 0), (0, 0, 0), 50.0, 4 / 254.0, 4 / 254.0, 100)
    assert (cam.x_pixels(), cam.y_pixels()) == (4, 4)
    planes = dict(color=np.zeros((4, 4, 3)), variance=np.zeros((4, 4)), weight=np.ones((4, 4)), normal=np.zeros((4, 4, 3)),
                  albedo=np.zeros((4, 4, 3)), depth=np.zeros((4, 4)), coverage=np.zeros((4, 4)), object=np.zeros((4, 4), np.uint32))

    def push(desc=cam.desc, hist=h, scalars=(8.0, 0.02, 0.25), **absent):
        ptr = [None if k in absent else planes[k].ctypes.data for k in T.PLANES]
        return L.rayrs_history_push_image(hist, None if desc is None else C.byref(desc), *ptr, *scalars)

    assert push(hist=None) == -1 and push(desc=None) == -1
    for k in T.PLANES:
        assert push(**{k: True}) == (-4 if k == "albedo" else -1), k        # albedo may be NULL
    for bad in (0.0, -1.0, INF, float("nan")):
        assert push(scalars=(bad, 0.02, 0.25)) == -1, bad
    for bad in (-1e-9, INF, float("nan")):
        assert push(scalars=(8.0, bad, 0.25)) == -1 and push(scalars=(8.0, 0.02, bad)) == -1, bad
    assert push(scalars=(8.0, 0.0, 0.0)) == -4
    empty, wide = _ffi.CameraDesc(), _ffi.CameraDesc()
    C.memmove(C.byref(empty), C.byref(cam.desc), C.sizeof(empty))
    C.memmove(C.byref(wide), C.byref(cam.desc), C.sizeof(wide))
    empty.x_pixels, wide.y_pixels = 0, 65536
    assert push(desc=empty) == -1 and push(desc=wide) == -5
    assert push(desc=wide, scalars=(0.0, 0.02, 0.25)) == -1      # a parameter refusal comes first
    assert push() == -4
    # an empty history answers nothing
    buf = np.zeros((4, 4, 3))
    assert L.rayrs_history_read(h, 1, buf.ctypes.data, None, None) == -1
    assert L.rayrs_history_read(None, 1, buf.ctypes.data, None, None) == -1
    assert L.rayrs_history_denoise_guided(h, 3, 1.0, 1.0, 1.0, 1.0, 1, buf.ctypes.data, None) == -1
    assert L.rayrs_history_push_times(h, (C.c_double * 5)()) == -1
    # a film: none to hand over without a device
    assert L.rayrs_history_push_film(h, None, 16, 8.0, 0.02, 0.25) == -1
    assert L.rayrs_history_push_film(None, None, 16, 8.0, 0.02, 0.25) == -1
    assert L.rayrs_history_reset(h) == 0 and L.rayrs_history_reset(None) == -1
    L.rayrs_history_destroy(h)
    L.rayrs_history_destroy(None)
    # the Python layer
    hist = rayrs_amd.History(device=-1)
    with pytest.raises(_ffi.RayrsError) as e:
        hist.push_image(cam, **planes)
    assert e.value.status == -4
    with pytest.raises(_ffi.RayrsError) as e:
        hist.image()
    assert e.value.status == -1
    with pytest.raises(ValueError):
        hist.push_image(cam, **dict(planes, depth=np.zeros((4, 5))))
    with pytest.raises(ValueError):
        hist.push_image(cam, **dict(planes, variance=None))


# ------------------------------------------------------------------------------------------------------ the orbit

def orbit_reading(origin, up, lookat, degrees):
    """The header's ORBIT lines with the oracle's sine and cosine; math.sqrt is IEEE's, as rr_sqrt is."""
    sin, cos = (lambda x: float(_oracle.lib().orc_math(0, x, 0.0))), (lambda x: float(_oracle.lib().orc_math(1, x, 0.0)))
    if degrees == 0.0:
        return list(origin)
    n2 = (up[0] * up[0] + up[1] * up[1]) + up[2] * up[2]
    inv = 1.0 / math.sqrt(n2)
    k = [up[i] * inv for i in range(3)]
    v = [origin[i] - lookat[i] for i in range(3)]
    rad = degrees * (math.pi / 180.0)
    c, s = cos(rad), sin(rad)
    kv = (k[0] * v[0] + k[1] * v[1]) + k[2] * v[2]
    g = kv * (1.0 - c)
    x = [k[1] * v[2] - k[2] * v[1], k[2] * v[0] - k[0] * v[2], k[0] * v[1] - k[1] * v[0]]
    return [lookat[i] + ((v[i] * c + x[i] * s) + k[i] * g) for i in range(3)]


@pytest.mark.parametrize("degrees", [0.0, 90.0, 360.0, 37.3, -123.456])
def test_the_orbit_is_the_headers_rotation_with_the_oracles_sine_and_cosine(degrees):
    L = _ffi.lib()
    for origin, up, lookat in (((0.0, 5.0, 10.0), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0)),
                               ((1.5, -2.25, 3.0), (0.3, 2.0, -0.4), (0.1, 0.2, 0.3))):
        out = (C.c_double * 3)()
        assert L.rayrs_camera_orbit(_oracle.d3(origin), _oracle.d3(up), _oracle.d3(lookat), degrees, out) == 0
        want = orbit_reading(origin, up, lookat, degrees)
        assert F.same_bits(np.array(out), np.array(want)), (degrees, list(out), want)
        # a rotation: the distance to the axis' foot and the height along it stay (to rounding)
        v0, v1 = np.subtract(origin, lookat), np.subtract(list(out), lookat)
        assert abs(np.linalg.norm(v0) - np.linalg.norm(v1)) < 1e-12 and abs(np.dot(v0, up) - np.dot(v1, up)) < 1e-12
        if degrees == 0.0:
            assert list(out) == list(origin)
    cam = rayrs_amd.Camera((0.0, 5.0, 10.0), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), 50.0, 0.1, 0.1, 100)
    moved = rayrs_amd.orbit(cam, degrees)
    assert list(moved.args[0]) == orbit_reading(*cam.args[:3], degrees) and moved.args[1:] == cam.args[1:]


def test_the_orbit_refuses_what_it_cannot_turn():
    L = _ffi.lib()
    o, out = _oracle.d3((0, 1, 5)), (C.c_double * 3)()
    assert L.rayrs_camera_orbit(o, _oracle.d3((0, 0, 0)), o, 10.0, out) == -1
    assert L.rayrs_camera_orbit(o, _oracle.d3((0, 1, 0)), o, INF, out) == -1
    assert L.rayrs_camera_orbit(None, _oracle.d3((0, 1, 0)), o, 1.0, out) == -1
    assert L.rayrs_camera_orbit(o, _oracle.d3((0, 1, 0)), o, 1.0, None) == -1


# ------------------------------------------------------------------------------------------------------ the reading

def test_the_readings_projection_inverts_the_oracles_primary_rays():
    """Every (pixel, sample) primary ray of the 32 x 24 sphere view: its points at t = 1 and t = 7.5 project back into the
    pixel -- fx within the jitter's range [col - 0.5, col + 0.5], fy likewise, widened by 1e-9 -- at tp = t to 1e-12."""
    cam_args = _film.sphere_desc()[0]
    ocam = _oracle.OracleCamera(*cam_args)
    cam = T.Cam(ocam.desc)
    h, w, samples = cam.H, cam.W, 8
    assert (w, h) == (_film.W, _film.H)
    checked = 0
    for r in range(h):
        for col in range(w):
            for s in range(samples):
                o, d, _ = ocam.primary_ray(h - r, w - col, path_key(_film.SEED, r * w + col, s))
                for t in (1.0, 7.5):
                    u = tuple((float(o[i]) + float(d[i]) * t) - cam.origin[i] for i in range(3))
                    sp, tp, fx, fy = T.project(cam, u)
                    assert sp > 0.0
                    assert col - 0.5 - 1e-9 <= fx <= col + 0.5 + 1e-9, (r, col, s, t, fx)
                    assert r - 0.5 - 1e-9 <= fy <= r + 0.5 + 1e-9, (r, col, s, t, fy)
                    assert abs(tp - t) <= 1e-12 * t, (r, col, s, t, tp)
                    checked += 1
    assert checked == h * w * samples * 2
    # and the centre ray is the primary ray with both jitters 0.5: its own pixel centre, to rounding
    for r, col in ((0, 0), (h - 1, w - 1), (7, 19)):
        sp, tp, fx, fy = T.project(cam, T.centre_ray(cam, r, col))
        assert abs(fx - col) < 1e-9 and abs(fy - r) < 1e-9 and abs(tp - 1.0) < 1e-12


def clean_view(cam, seed):
    """analytic_view without the awkward values."""
    view = T.analytic_view(cam, seed)
    bad = ~np.isfinite(view["color"]).all(axis=2)
    view["color"][bad] = 0.5
    view["variance"][~(view["variance"] >= 0.0) | (view["variance"] == INF)] = 0.01
    view["weight"][view["weight"] == 0.0] = 8.0
    view["coverage"][np.isnan(view["coverage"])] = 0.0
    return view


def test_without_a_valid_tap_the_frames_own_bits_come_back():
    args = T.pairs(33, 17)
    cam_a, cam_b, away = T.oracle_cam(args[1][1]), T.oracle_cam(args[1][2]), T.oracle_cam(args[4][2])
    a, b = T.analytic_view(cam_a, 1), T.analytic_view(cam_b, 2)
    blendable = np.isfinite(a["color"]).all(axis=2) & (a["weight"] > 0.0)

    def unchanged(out):
        return all(F.same_bits(out[k][blendable], a[k][blendable]) for k in ("color", "variance", "weight"))

    # object planes that differ everywhere (and no background to agree on)
    b2 = dict(b, coverage=np.ones_like(b["coverage"]), object=np.full(b["object"].shape, 7, dtype=np.uint32))
    out, tally = T.push(cam_a, a, cam_b, b2, 40.0, 0.02, 0.25)
    assert unchanged(out) and tally["blended"] == 0 and tally["tap_object"] > 0 and tally["tap_not_background"] > 0
    # B facing away
    out, tally = T.push(cam_a, a, away, T.analytic_view(away, 3), 40.0, 0.02, 0.25)
    assert unchanged(out) and tally["blended"] == 0 and tally["behind"] == int(blendable.sum()) - tally["no_source"]
    # an empty history; passed-through pixels keep colour and variance, and their weight is wc or +0
    out, tally = T.push(cam_a, a, None, None, 40.0, 0.02, 0.25)
    assert unchanged(out) and tally["empty"] == int(blendable.sum()) and tally["pass_through"] == int((~blendable).sum())
    assert F.same_bits(out["color"], a["color"]) and F.same_bits(out["variance"], a["variance"])
    assert F.same_bits(out["weight"][~blendable], np.where(a["weight"] > 0.0, a["weight"], 0.0)[~blendable])


def test_constant_planes_under_one_camera_give_the_constant_and_the_capped_weight():
    cam = T.oracle_cam(T.pairs(33, 17)[0][1])
    b = clean_view(cam, 5)
    b["color"][:] = (0.25, 0.5, 0.75)
    b["variance"][:] = 0.01
    a = dict(b, weight=np.full_like(b["weight"], 8.0))
    for cap in (16.0, 1000.0):
        out, tally = T.push(cam, a, cam, b, cap, 0.02, 0.25)
        assert tally["blended"] == cam.W * cam.H and (tally["cap_active"] > 0) == (cap == 16.0)
        assert np.abs(out["color"] - (0.25, 0.5, 0.75)).max() <= 1e-15
        assert np.abs(out["weight"] - (np.minimum(b["weight"], cap) + 8.0)).max() <= 1e-12
        assert (out["variance"] < 0.01).all()             # two independent estimates: less noise than either


def test_an_all_infinite_incoming_variance_over_a_finite_history_comes_out_finite():
    cam = T.oracle_cam(T.pairs(33, 17)[0][1])
    b = clean_view(cam, 6)
    a = dict(clean_view(cam, 7), variance=np.full((cam.H, cam.W), INF))
    out, tally = T.push(cam, a, cam, b, 40.0, 0.02, 0.25)
    assert tally["heal_frame"] == tally["blended"] > 0 and tally["heal_history"] == 0
    healed = ~F_same_plane(out["variance"], a["variance"])
    assert healed.sum() == tally["blended"] and np.isfinite(out["variance"][healed]).all()
    # and the other way round: an infinite history under a finite frame
    out, tally = T.push(cam, clean_view(cam, 7), cam, dict(b, variance=np.full((cam.H, cam.W), INF)), 40.0, 0.02, 0.25)
    assert tally["heal_history"] == tally["blended"] > 0 and np.isfinite(out["variance"]).all()
    # both infinite: it stays so, and no NaN is made
    out, tally = T.push(cam, a, cam, dict(b, variance=np.full((cam.H, cam.W), INF)), 40.0, 0.02, 0.25)
    assert (out["variance"] == INF).all() and not np.isnan(out["color"]).any()


def F_same_plane(x, y):
    return x.view(np.uint64) == y.view(np.uint64)


def test_the_gpu_tests_case_list_takes_every_branch_of_the_reading():
    """What keeps the bit-for-bit comparison of test_gpu_temporal.py from being vacuous."""
    total = dict.fromkeys(T.BRANCHES, 0)
    for size in T.SIZES:
        for pair in range(len(T.pairs(*size))):
            case = T.image_case(size, pair)
            for branch in T.BRANCHES:
                total[branch] += case["tally"][branch]
            if case["name"] != "identical":
                assert (T.oracle_cam(case["args"]["b"]).W, T.oracle_cam(case["args"]["b"]).H) != size, case["name"]
            # no case makes a NaN of its own: bit patterns are comparable across machines
            for (_, view), state in zip(case["pushes"], case["states"]):
                assert (np.isnan(state["color"]) == np.isnan(view["color"])).all()
                assert (np.isnan(state["variance"]) <= np.isnan(view["variance"])).all() and not np.isnan(state["weight"]).any()
    assert all(total[b] > 0 for b in T.BRANCHES), {b: n for b, n in total.items() if n == 0}
    assert (T.oracle_cam(T.image_case((1, 1), 0)["args"]["a"]).W, T.oracle_cam(T.image_case((65, 5), 0)["args"]["a"]).H) == (1, 5)


# ------------------------------------------------------------------------------------------------------ the kernel

needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@needs_hipcc
def test_the_reprojection_kernel_fits_four_waves_per_simd(tmp_path):
    """at most 128 vector registers, no scratch, no LDS."""
    res = kernel_resources(compile_asm("temporal.hip", tmp_path))
    (name, (vgpr, scratch, lds)), = res.items()
    assert "temporal_kernel" in name
    assert vgpr <= 128 and scratch == 0 and lds == 0, (name, vgpr, scratch, lds)
