"""Temporal accumulation on the GPU (include/rayrs_hip.h TEMPORAL ACCUMULATION), held bit for bit to the plain-Python reading
of tests/_temporal.py: rayrs_history_push_image on analytic views with the awkward values in -- every size and camera pair
of _temporal's case list (which test_temporal.py shows to take every branch of the reading), three pushes deep, all three
planes in both output formats --; rayrs_history_push_film against the reading applied to inputs derived from the oracle
alone, uniform, after an adaptive pass and with a one-chunk film, the films untouched by it; the history through the guided
filter against _guided.py; the command line's orbit."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import _features as F
import _film
import _film_adaptive as A
import _guided as G
import _temporal as T
import rayrs_amd
from rayrs_amd import _ffi, io, procedural, scenes

pytestmark = pytest.mark.gpu

SEED, BOUNCES, CHUNK = _film.SEED, _film.BOUNCES, _film.C
CLI = os.path.join(os.path.dirname(os.path.abspath(rayrs_amd.__file__)), "rayrs")
INF = float("inf")


def assert_same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if not F.same_bits(got, want):
        view = {8: np.uint64, 4: np.uint32}[got.dtype.itemsize]
        bad = got.view(view) != want.view(view)
        bad = bad.any(axis=2) if bad.ndim == 3 else bad
        y, x = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} pixels differ; first at ({y}, {x}): {got[y, x]} != {want[y, x]}")


def read_all(hist, cam, f64):
    """rayrs_history_read: the three planes in one output format."""
    dt = np.float64 if f64 else np.float32
    h, w = cam.y_pixels(), cam.x_pixels()
    c, v, m = np.full((h, w, 3), 7, dtype=dt), np.full((h, w), 7, dtype=dt), np.full((h, w), 7, dtype=dt)
    _ffi.check(_ffi.lib().rayrs_history_read(hist._h, 1 if f64 else 0, c.ctypes.data, v.ctypes.data, m.ctypes.data), "rayrs_history_read")
    return c, v, m


def assert_history(hist, cam, state, what):
    for f64 in (True, False):
        got = read_all(hist, cam, f64)
        for plane, g in zip(("color", "variance", "weight"), got):
            with np.errstate(over="ignore", invalid="ignore"):
                want = state[plane] if f64 else state[plane].astype(np.float32)
            assert_same(g, want, (what, plane, "f64" if f64 else "f32"))


# ------------------------------------------------------------------------------------------------------ image level

@pytest.mark.parametrize("size", T.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pushed_images_equal_the_reading_three_pushes_deep(size):
    for pair in range(len(T.pairs(*size))):
        case = T.image_case(size, pair)
        cams = {k: rayrs_amd.Camera(*case["args"][k]) for k in ("a", "b")}
        for k, cam in cams.items():   # the library's camera is the oracle's, to the bit: the reading and the kernel see one view
            ocam = T.oracle_cam(case["args"][k])
            for field in ("origin", "e_x", "e_y", "z"):
                assert tuple(getattr(cam.desc, field)) == getattr(ocam, field), (case["name"], k, field)
        hist = rayrs_amd.History(device=0)
        for n, ((key, view), state) in enumerate(zip(case["pushes"], case["states"])):
            hist.push_image(cams[key], max_samples=T.MAX_WEIGHT, depth_tol=T.DEPTH_TOL, normal_tol=T.NORMAL_TOL,
                            **{p: view[p] for p in T.PLANES})
            assert_history(hist, cams[key], state, (size, case["name"], "push", n))
        # each plane may be left out of a read, and albedo of a push: the same history
        assert_same(hist.image(out_f64=True), case["states"][2]["color"], (size, case["name"], "image"))
        assert_same(hist.variance(), case["states"][2]["variance"], (size, case["name"], "variance"))
        assert_same(hist.weight(), case["states"][2]["weight"], (size, case["name"], "weight"))
        hist.reset()
        with pytest.raises(_ffi.RayrsError):
            hist.image()
        hist.push_image(cams["b"], **dict({p: case["pushes"][0][1][p] for p in T.PLANES}, albedo=None), max_samples=T.MAX_WEIGHT)
        assert_history(hist, cams["b"], case["states"][0], (size, case["name"], "after a reset"))


# ------------------------------------------------------------------------------------------------------ film level

MOVE = (0.6, 0.0, -0.1)     # the second camera's origin, from the first's
FILM_CAP = 6.0              # below the first film's weight: the cap is active


def descs(name):
    """The scene's description from its own camera and from the moved one."""
    cam_args, objs, heur, env = _film.DESCS[name]()
    origin = tuple(o + d for o, d in zip(cam_args[0], MOVE))
    return (cam_args, objs, heur, env), ((origin,) + tuple(cam_args[1:]), objs, heur, env)


@functools.lru_cache(maxsize=None)
def oracle_inputs(name, which):
    """Per-sample radiance and iteration counts (20 samples) and the features of 16 samples of the view, from the oracle."""
    desc = descs(name)[which]
    rgb, it = A.traces(*_film.oracle_of(desc), 20)
    feats = F.named_samples(name, 16) if which == 0 else F.sample_features(desc, 16)
    return desc, rgb, it, F.features_from(feats, 16)


def oracle_view(name, which, passes):
    """The view a film pushes after `passes` -- ("uniform", n) or ("adaptive", n, tau, cap) -- from the oracle alone: the
    frame and S1, S2 of _film.expectation per tile count, the noise plane of _guided, the weight N_t, the features."""
    desc, rgb, it, feats = oracle_inputs(name, which)
    rep = A.Replay(rgb, it)
    for p in passes:
        rep.uniform_pass(p[1]) if p[0] == "uniform" else rep.adaptive_pass(*p[1:])
    s1, s2 = rep.sums()
    view = dict(feats, color=rep.frame(), variance=G.noise_plane(s1, s2, rep.nt, CHUNK),
                weight=rep.per_pixel(rep.nt).astype(np.float64))
    return view, rep


def run_film(scene, cam, passes):
    film = rayrs_amd.Film(scene, cam, sample_chunk=CHUNK, max_bounces=BOUNCES, seed=SEED)
    for p in passes:
        film.render(p[1]) if p[0] == "uniform" else film.render_adaptive(*p[1:])
    return film


UNIFORM = (("uniform", 8),)
ADAPTIVE = (("uniform", 16), ("adaptive", 4, 0.6, 24))   # (test_gpu_guided.py's: it leaves the tiles at 16 and 20)
ONE_CHUNK = (("uniform", 4),)


@pytest.mark.parametrize("name", ["sphere", "mesh"])
@pytest.mark.parametrize("second", [UNIFORM, ADAPTIVE, ONE_CHUNK], ids=["uniform", "adaptive", "one chunk"])
def test_pushed_films_equal_the_reading_of_the_oracles_planes(name, second):
    (desc_a, desc_b) = descs(name)
    scene = rayrs_amd.Scene(desc_a[1], 1e-6, 1e6, desc_a[2], desc_a[3], device=0)
    cams = [rayrs_amd.Camera(*desc_a[0]), rayrs_amd.Camera(*desc_b[0])]
    ocams = [T.oracle_cam(desc_a[0]), T.oracle_cam(desc_b[0])]
    first = ADAPTIVE if second is ADAPTIVE else UNIFORM
    hist = rayrs_amd.History(device=0)
    state, state_cam = None, None
    for which, passes in ((0, first), (1, second)):
        film = run_film(scene, cams[which], passes)
        view, rep = oracle_view(name, which, passes)
        assert np.array_equal(film.tile_samples(), rep.nt)
        if passes is ADAPTIVE:
            assert len(np.unique(rep.nt)) > 1, "the adaptive pass left every tile alike: pick another tau"
        if passes is ONE_CHUNK:
            assert (view["variance"] == INF).all()
        before = (film.image(out_f64=True), film.status(0.2), film.state())
        hist.push(film, feature_samples=16, max_samples=FILM_CAP, depth_tol=T.DEPTH_TOL, normal_tol=T.NORMAL_TOL)
        state, tally = T.push(ocams[which], view, state_cam, state, FILM_CAP, T.DEPTH_TOL, T.NORMAL_TOL)
        state_cam = ocams[which]
        assert_history(hist, cams[which], state, (name, which))
        # the film is as it was
        assert F.same_bits(film.image(out_f64=True), before[0]) and film.status(0.2) == before[1] and film.state() == before[2]
        times = hist.push_times()
        assert len(times) == 5 and all(t >= 0.0 for t in times.values())
    # the second push did reproject (these views are all surface: no background), under the cap
    assert tally["hit_tap"] > 0 and tally["blended"] > 100 and tally["cap_active"] > 0
    if second is ONE_CHUNK:
        assert tally["heal_frame"] == tally["blended"] and np.isfinite(state["variance"]).sum() >= tally["blended"]
    assert not F.same_bits(state["color"], view["color"])


def test_film_refusals_with_a_device():
    desc = descs("sphere")[0]
    scene, cam = rayrs_amd.Scene(desc[1], 1e-6, 1e6, desc[2], desc[3], device=0), rayrs_amd.Camera(*desc[0])
    L, hist = _ffi.lib(), rayrs_amd.History(device=0)
    film = rayrs_amd.Film(scene, cam, sample_chunk=CHUNK, max_bounces=BOUNCES, seed=SEED)
    push = lambda f=film, h=hist, fs=16, mw=8.0, dt=0.02, nt=0.25: L.rayrs_history_push_film(h._h, f._h, fs, mw, dt, nt)  # noqa: E731
    assert push() == -1                                   # an empty film
    film.render(4)
    assert push(fs=0) == -1 and push(mw=0.0) == -1 and push(mw=INF) == -1 and push(dt=-1.0) == -1 and push(nt=float("nan")) == -1
    share = rayrs_amd.Film(scene, cam, sample_chunk=CHUNK, max_bounces=BOUNCES, seed=SEED, tile_rank=0, tile_ranks=2)
    share.render(4)
    assert push(f=share) == -1                            # reprojection reads a pixel's neighbours
    assert push(h=rayrs_amd.History(device=-1)) == -1     # a film on another device than the history
    assert L.rayrs_history_push_times(hist._h, (C.c_double * 5)()) == -1   # nothing was pushed
    assert push() == 0 and L.rayrs_history_push_times(hist._h, (C.c_double * 5)()) == 0
    buf = np.zeros((cam.y_pixels(), cam.x_pixels(), 3))
    assert L.rayrs_history_read(hist._h, 2, buf.ctypes.data, None, None) == -1
    assert L.rayrs_history_read(hist._h, 1, None, None, None) == 0
    for bad in (dict(levels=0), dict(levels=17), dict(kv=-1.0), dict(ka=float("nan")), dict(fmt=2), dict(out=None)):
        kw = dict(dict(levels=3, kn=1.0, ka=1.0, kz=1.0, kv=1.0, fmt=1, out=buf.ctypes.data), **bad)
        assert L.rayrs_history_denoise_guided(hist._h, kw["levels"], kw["kn"], kw["ka"], kw["kz"], kw["kv"], kw["fmt"], kw["out"], None) == -1, bad
    assert L.rayrs_history_denoise_guided(hist._h, 3, 1.0, 1.0, 1.0, 1.0, 1, buf.ctypes.data, None) == 0


# ------------------------------------------------------------------------------------------------------ the filter

SIGMAS = dict(sigma_normal=0.5, sigma_albedo=0.2, sigma_depth=2.0, sigma_luminance=4.0)


def test_the_history_through_the_guided_filter_equals_the_reference():
    desc_a, desc_b = descs("sphere")
    scene = rayrs_amd.Scene(desc_a[1], 1e-6, 1e6, desc_a[2], desc_a[3], device=0)
    films = [run_film(scene, rayrs_amd.Camera(*d[0]), UNIFORM) for d in (desc_a, desc_b)]
    for film, hist in zip(films, [rayrs_amd.History(device=0)] * 2):
        hist.push(film)
    color, variance, weight = hist.read()
    assert np.isfinite(variance).all() and (weight > 8.0).any()
    feats = films[1].features(16)
    k = [F.k_of(SIGMAS[s]) for s in ("sigma_normal", "sigma_albedo", "sigma_depth", "sigma_luminance")]
    want, want_var = G.guided(color, variance, feats["normal"], feats["albedo"], feats["depth"], 2, *k)
    got, got_var = hist.denoised_guided(levels=2, out_f64=True, return_variance=True, **SIGMAS)
    assert_same(got, want, "guided history")
    assert_same(got_var, want_var, "guided history variance")
    assert not F.same_bits(got, color)
    got32 = hist.denoised_guided(levels=2, **SIGMAS)
    assert got32.dtype == np.float32 and F.same_bits(got32, want.astype(np.float32))
    assert hist.denoised_guided().shape == color.shape        # the defaults run, with the scene's depth sigma
    # the history is as it was
    for a, b in zip(hist.read(), (color, variance, weight)):
        assert F.same_bits(a, b)
    # render_sequence is the same two pushes
    seq = list(rayrs_amd.render_sequence(scene, [f.camera for f in films], 8, sample_chunk=CHUNK, max_bounces=BOUNCES, seed=SEED))
    assert len(seq) == 2 and seq[0][1] is seq[1][1]
    for a, b in zip(seq[1][1].read(), (color, variance, weight)):
        assert F.same_bits(a, b)


# ------------------------------------------------------------------------------------------------------ the command line

def run_cli(tmp, sub, args, status=0):
    d = tmp / sub
    d.mkdir()
    r = subprocess.run([CLI, str(tmp / "env.hdr"), "8", "--seed", "77"] + args, cwd=d, capture_output=True, text=True, timeout=600)
    assert r.returncode == status, (r.returncode, r.stderr)
    return d


def test_the_command_lines_orbit(tmp_path):
    io.save_hdr(tmp_path / "env.hdr", procedural.make_hdri(128, 64))
    plain = run_cli(tmp_path, "plain", ["--pass", "8"])
    orbit = run_cli(tmp_path, "orbit", ["--orbit", "3", "20", "--pass", "8", "--temporal"])
    names = [f"material_test_{i:04d}{kind}.{ext}" for i in range(3) for kind in ("", "_temporal") for ext in ("hdr", "png")]
    assert sorted(os.listdir(orbit)) == sorted(names)
    for ext in ("hdr", "png"):   # frame 0 is the plain run's frame, and its history the frame itself
        assert (orbit / f"material_test_0000.{ext}").read_bytes() == (plain / f"material_test.{ext}").read_bytes(), ext
        assert (orbit / f"material_test_0000_temporal.{ext}").read_bytes() == (plain / f"material_test.{ext}").read_bytes(), ext
    # no film: a usage error, status 2, nothing written
    for k, flags in enumerate((["--orbit", "3", "20"], ["--orbit", "3", "20", "--temporal"], ["--temporal", "--pass", "8"])):
        assert os.listdir(run_cli(tmp_path, f"refused{k}", flags, status=2)) == []
    # the library, same scene, same HDRI as decoded from the file, the same cameras
    cam_args, objs, heur = scenes.material_test()
    env = io.load_hdr(tmp_path / "env.hdr")
    scene, cam = rayrs_amd.Scene(objs, 1e-6, 1e6, heur, env, device=0), rayrs_amd.Camera(*cam_args)
    cams = [rayrs_amd.orbit(cam, i * 20.0 / 3.0) for i in range(2)]
    assert cams[0].args == cam.args
    for i, (film, hist) in enumerate(rayrs_amd.render_sequence(scene, cams, 8, sample_chunk=4, max_bounces=50, seed=77)):
        io.save_hdr(tmp_path / "want.hdr", film.image())
        assert (orbit / f"material_test_{i:04d}.hdr").read_bytes() == (tmp_path / "want.hdr").read_bytes(), i
        io.save_hdr(tmp_path / "want_temporal.hdr", hist.image())
        assert (orbit / f"material_test_{i:04d}_temporal.hdr").read_bytes() == (tmp_path / "want_temporal.hdr").read_bytes(), i
    assert not F.same_bits(hist.image(), film.image())        # frame 1's history is more than frame 1
