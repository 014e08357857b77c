"""The film's noise plane and the variance-guided a-trous filter on the GPU (include/rayrs_hip.h NOISE PLANE, GUIDED FILTER),
held bit for bit to the plain-Python reference of tests/_guided.py: rayrs_image_denoise_guided on seeded random frames and
variance planes with the awkward values in, every level count up to steps beyond the image, every k switched off and every
plane absent in turn, the all-infinite plane against the feature-guided filter on the GPU itself; a film's plane and
guided frame against the reference applied to the oracle's S1, S2 and features, uniform, after an adaptive pass, with one
chunk, closed, and on a tile share; both filters in turn on one film's shared buffers; the command line's extra files."""
import os
import subprocess

import numpy as np
import pytest

import _features as F
import _film
import _film_adaptive as A
import _guided as G
import rayrs_amd
from rayrs_amd import _ffi, io, procedural, scenes

pytestmark = pytest.mark.gpu

SEED, BOUNCES, C = _film.SEED, _film.BOUNCES, _film.C
CLI = os.path.join(os.path.dirname(os.path.abspath(rayrs_amd.__file__)), "rayrs")
K = (4.0, 25.0, 0.3, 0.0625)   # kn, ka, kz, kv
SIGMAS = dict(sigma_normal=0.5, sigma_albedo=0.2, sigma_depth=2.0, sigma_luminance=4.0)
INF = float("inf")


def gpu_guided(color, var, normal, albedo, depth, levels, kn, ka, kz, kv):
    """rayrs_image_denoise_guided with the k themselves: (colour, variance)."""
    L = _ffi.lib()
    color = np.ascontiguousarray(color, dtype=np.float64)
    var = np.ascontiguousarray(var, dtype=np.float64)
    h, w = color.shape[:2]
    out, out_var = np.full((h, w, 3), 7.0), np.full((h, w), 7.0)
    keep = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (normal, albedo, depth)]
    ptr = [None if a is None else a.ctypes.data for a in keep]
    _ffi.check(L.rayrs_image_denoise_guided(0, w, h, color.ctypes.data, var.ctypes.data, ptr[0], ptr[1], ptr[2], levels, kn, ka, kz,
                                            kv, out.ctypes.data, out_var.ctypes.data), "rayrs_image_denoise_guided")
    return out, out_var


def assert_same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if not F.same_bits(got, want):
        bad = got.view(np.uint64) != want.view(np.uint64)
        bad = bad.any(axis=2) if bad.ndim == 3 else bad
        y, x = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} pixels differ; first at ({y}, {x}): {got[y, x]} != {want[y, x]}")


@pytest.mark.parametrize("size", [(1, 1), (7, 5), (65, 5), (33, 17), (64, 48)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_filter_equals_the_reference_at_every_level_count(size):
    w, h = size
    color, normal, albedo, depth = F.random_case(200 + w, w, h)
    var = G.random_variance(300 + w, w, h)
    if w * h >= 8:
        assert not np.isfinite(color).all() and np.isnan(var).sum() == 1 and (var < 0).sum() == 1 and (var == INF).any()
    for levels, (want, want_var) in enumerate(G.guided_levels(color, var, normal, albedo, depth, 6, *K), start=1):   # step 32 at the last
        got, got_var = gpu_guided(color, var, normal, albedo, depth, levels, *K)
        assert_same(got, want, (size, levels, "colour"))
        assert_same(got_var, want_var, (size, levels, "variance"))
    # the Python entry point with sigmas whose k are exact
    got, got_var = rayrs_amd.denoise_guided(color, var, normal, albedo, depth, levels=2, sigma_normal=0.5, sigma_albedo=0.25,
                                            sigma_depth=2.0, sigma_luminance=4.0, return_variance=True)
    want, want_var = G.guided(color, var, normal, albedo, depth, 2, 4.0, 16.0, 0.25, 0.0625)
    assert_same(got, want, (size, "sigmas"))
    assert_same(got_var, want_var, (size, "sigmas", "variance"))
    assert_same(rayrs_amd.denoise_guided(color, var, normal, albedo, depth, levels=2, sigma_normal=0.5, sigma_albedo=0.25,
                                         sigma_depth=2.0), want, (size, "no variance asked for"))


def test_each_k_switched_off_and_each_plane_absent_in_turn():
    w, h = 33, 17
    color, normal, albedo, depth = F.random_case(5, w, h)
    var = G.random_variance(6, w, h)

    def check(planes, k, what):
        got, got_var = gpu_guided(color, var, *planes, 3, *k)
        want, want_var = G.guided(color, var, *planes, 3, *k)
        assert_same(got, want, what)
        assert_same(got_var, want_var, (what, "variance"))

    planes = [normal, albedo, depth]
    for i in range(4):
        k = list(K)
        k[i] = 0.0
        check(planes, k, ("k", i))
    for i in range(3):
        p = list(planes)
        p[i] = None
        check(p, K, ("plane", i))
    check([None, None, None], K, "no plane")


def test_an_all_infinite_variance_is_the_feature_guided_filter_on_the_gpu():
    w, h = 33, 17
    color, normal, albedo, depth = F.random_case(7, w, h)
    var = np.full((h, w), INF)
    L = _ffi.lib()
    for levels in (1, 4):
        plain = np.zeros((h, w, 3))
        _ffi.check(L.rayrs_image_denoise(0, w, h, color.ctypes.data, normal.ctypes.data, albedo.ctypes.data, depth.ctypes.data, levels,
                                         K[0], K[1], K[2], 0.0, plain.ctypes.data), "rayrs_image_denoise")
        got, got_var = gpu_guided(color, var, normal, albedo, depth, levels, *K)
        assert_same(got, plain, ("kc = 0", levels))
        assert not np.isnan(got_var).any() and (got_var == INF).all()


# ------------------------------------------------------------------------------------------------------ the film

def make_film(name, **kw):
    cam_args, objs, heur, env = _film.DESCS[name]()
    scene, cam = rayrs_amd.Scene(objs, 1e-6, 1e6, heur, env, device=0), rayrs_amd.Camera(*cam_args)
    return scene, cam, rayrs_amd.Film(scene, cam, sample_chunk=C, max_bounces=BOUNCES, seed=SEED, **kw)


def replay(name, **kw):
    rgb, it = A.named_traces(name, 24, _film.W, _film.H)
    return A.Replay(rgb, it, **kw)


def features(name):
    return F.features_from(F.named_samples(name, 16), 16)


def k_of_sigmas():
    return [F.k_of(SIGMAS[s]) for s in ("sigma_normal", "sigma_albedo", "sigma_depth", "sigma_luminance")]


@pytest.mark.parametrize("name", ["sphere", "mesh"])
def test_a_films_plane_and_guided_frame_equal_the_reference_after_an_adaptive_pass(name):
    scene, cam, film = make_film(name)
    rep = replay(name)
    film.render(16)
    rep.uniform_pass(16)
    active, _ = film.render_adaptive(4, 0.6, 24)
    p = rep.adaptive_pass(4, 0.6, 24)
    per_tile = film.tile_samples()
    assert active == p["active_tiles"] and np.array_equal(per_tile, rep.nt)
    assert 0 < active < per_tile.size and len(np.unique(per_tile)) > 1, "the adaptive pass left every tile alike: pick another tau"
    frame, status, state = film.image(out_f64=True), film.status(0.2), film.state()

    plane = G.noise_plane(p["s1"], p["s2"], rep.nt, C)
    assert np.isfinite(plane).all() and (plane > 0).any()
    assert_same(film.noise(), plane, (name, "noise"))
    feats = features(name)
    want, want_var = G.guided(frame, plane, feats["normal"], feats["albedo"], feats["depth"], 3, *k_of_sigmas())
    got, got_var = film.denoised_guided(levels=3, feature_samples=16, out_f64=True, return_variance=True, **SIGMAS)
    assert_same(got, want, (name, "guided"))
    assert_same(got_var, want_var, (name, "guided variance"))
    assert not F.same_bits(got, frame)                            # it did filter
    assert not F.same_bits(got, film.denoised(levels=3, feature_samples=16, out_f64=True, sigma_normal=0.5, sigma_albedo=0.2,
                                              sigma_depth=2.0, sigma_color=None))   # and the variance did guide
    got32 = film.denoised_guided(levels=3, feature_samples=16, **SIGMAS)
    assert got32.dtype == np.float32 and F.same_bits(got32, want.astype(np.float32)), (name, "f32")
    # the film is as it was
    assert F.same_bits(film.image(out_f64=True), frame) and film.status(0.2) == status and film.state() == state
    # the defaults run
    assert film.denoised_guided().shape == (cam.y_pixels(), cam.x_pixels(), 3)


def test_with_one_chunk_the_plane_is_infinite_and_the_filter_the_feature_guided_one():
    scene, cam, film = make_film("sphere")
    film.render(4)
    plane = film.noise()
    assert (plane == INF).all()
    got, got_var = film.denoised_guided(levels=4, out_f64=True, return_variance=True)
    assert_same(got, film.denoised(levels=4, sigma_color=None, out_f64=True), "M = 1")
    assert (got_var == INF).all()


def test_a_closed_film_still_answers():
    scene, cam, film = make_film("sphere")
    film.render(8), film.render(2)
    assert film.status()["closed"] == 1
    rgb, _ = A.named_traces("sphere", 24, _film.W, _film.H)
    frame, s1, s2, m = _film.expectation(rgb, C, 10)
    assert m == 2
    plane = G.noise_plane(s1, s2, np.full(((_film.H + 7) // 8, (_film.W + 7) // 8), 10), C)   # the short chunk is not in it
    assert_same(film.noise(), plane, "closed noise")
    assert_same(film.image(out_f64=True), frame, "closed frame")
    feats = features("sphere")
    want, want_var = G.guided(frame, plane, feats["normal"], feats["albedo"], feats["depth"], 2, *k_of_sigmas())
    got, got_var = film.denoised_guided(levels=2, feature_samples=16, out_f64=True, return_variance=True, **SIGMAS)
    assert_same(got, want, "closed guided")
    assert_same(got_var, want_var, "closed guided variance")


def test_a_tile_share_reads_zero_outside_and_refuses_the_filter():
    scene, cam, film = make_film("sphere", tile_rank=1, tile_ranks=2)
    rep = replay("sphere", rank=1, ranks=2)
    L = _ffi.lib()
    buf = np.zeros((cam.y_pixels(), cam.x_pixels(), 3))
    plane_buf = np.zeros((cam.y_pixels(), cam.x_pixels()))
    # an empty film: both calls are refused
    assert L.rayrs_film_noise(film._h, plane_buf.ctypes.data) == -1
    assert L.rayrs_film_denoise_guided(film._h, 16, 3, 1.0, 1.0, 1.0, 1.0, 1, buf.ctypes.data, None) == -1
    film.render(8)
    p = rep.uniform_pass(8)
    plane = G.noise_plane(p["s1"], p["s2"], rep.nt, C, rep.share)
    outside = ~rayrs_amd.tiles.tile_mask(cam.x_pixels(), cam.y_pixels(), 1, 2)
    assert outside.any() and (plane[outside] == 0.0).all() and (plane[~outside] > 0.0).any()
    assert_same(film.noise(), plane, "share noise")
    assert L.rayrs_film_noise(film._h, None) == -1
    assert L.rayrs_film_denoise_guided(film._h, 16, 3, 1.0, 1.0, 1.0, 1.0, 1, buf.ctypes.data, None) == -1
    with pytest.raises(_ffi.RayrsError) as e:
        film.denoised_guided()
    assert e.value.status == -1
    # and on a whole film the parameter refusals
    scene2, cam2, whole = make_film("sphere")
    whole.render(4)
    h = whole._h
    assert L.rayrs_film_denoise_guided(h, 16, 0, 1.0, 1.0, 1.0, 1.0, 1, buf.ctypes.data, None) == -1
    assert L.rayrs_film_denoise_guided(h, 16, 17, 1.0, 1.0, 1.0, 1.0, 1, buf.ctypes.data, None) == -1
    assert L.rayrs_film_denoise_guided(h, 16, 3, 1.0, 1.0, 1.0, -1.0, 1, buf.ctypes.data, None) == -1
    assert L.rayrs_film_denoise_guided(h, 16, 3, 1.0, float("nan"), 1.0, 1.0, 1, buf.ctypes.data, None) == -1
    assert L.rayrs_film_denoise_guided(h, 0, 3, 1.0, 1.0, 1.0, 1.0, 1, buf.ctypes.data, None) == -1
    assert L.rayrs_film_denoise_guided(h, 16, 3, 1.0, 1.0, 1.0, 1.0, 2, buf.ctypes.data, None) == -1
    assert L.rayrs_film_denoise_guided(h, 16, 3, 1.0, 1.0, 1.0, 1.0, 1, None, None) == -1
    assert L.rayrs_film_denoise_guided(h, 16, 3, 1.0, 1.0, 1.0, 1.0, 1, buf.ctypes.data, None) == 0


def test_the_two_filters_share_a_films_buffers_without_a_trace_of_each_other():
    """A film works both filters in one set of buffers, whose frames the two lay out differently (24-byte colours, 32-byte
    records): alternating them, with level counts that end in either frame and each output form, every result is, bit for
    bit, what the same call gives as the first on a fresh film."""
    cam_args, objs, heur, env = _film.DESCS["sphere"](33, 17)
    scene, cam = rayrs_amd.Scene(objs, 1e-6, 1e6, heur, env, device=0), rayrs_amd.Camera(*cam_args)

    def new_film():
        film = rayrs_amd.Film(scene, cam, sample_chunk=C, max_bounces=BOUNCES, seed=SEED)
        film.render(2 * C)
        return film

    calls = [("denoised", dict(levels=3)),
             ("denoised_guided", dict(levels=2, return_variance=True)),
             ("denoised", dict(levels=1, out_f64=True)),
             ("denoised_guided", dict(levels=3)),
             ("denoised", dict(levels=2))]
    film = new_film()
    assert np.isfinite(film.noise()).all()                       # two full chunks: the variance does guide
    for i, (method, kw) in enumerate(calls):
        got, want = getattr(film, method)(**kw), getattr(new_film(), method)(**kw)
        if not isinstance(got, tuple):
            got, want = (got,), (want,)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and g.shape == w.shape and F.same_bits(g, w), (i, method, kw)


# ------------------------------------------------------------------------------------------------------ the command line

def run_cli(tmp, sub, args, status=0):
    d = tmp / sub
    d.mkdir()
    r = subprocess.run([CLI, str(tmp / "env.hdr"), "8", "--seed", "77"] + args, cwd=d, capture_output=True, text=True, timeout=600)
    assert r.returncode == status, (r.returncode, r.stderr)
    return d


def test_the_command_line_writes_the_guided_and_noise_files_only_when_asked(tmp_path):
    io.save_hdr(tmp_path / "env.hdr", procedural.make_hdri(128, 64))
    mode = ["--sample-chunk", "4", "--pass", "4"]
    plain = run_cli(tmp_path, "without", mode)
    extra = run_cli(tmp_path, "with", mode + ["--denoise-guided", "3", "--noise"])
    ordinary = ["material_test.hdr", "material_test.png"]
    new = ["material_test_guided.hdr", "material_test_guided.png", "material_test_noise.hdr"]
    assert sorted(os.listdir(plain)) == ordinary
    assert sorted(os.listdir(extra)) == sorted(ordinary + new)
    for name in ordinary:
        assert (plain / name).read_bytes() == (extra / name).read_bytes(), name
    # one flag, one kind of file; the level count is optional
    only = run_cli(tmp_path, "only", ["--denoise-guided"] + mode)
    assert sorted(os.listdir(only)) == sorted(ordinary + new[:2])
    # no film: a usage error, status 2, nothing written
    for k, flags in enumerate((["--noise"], ["--denoise-guided", "3"], ["--sample-chunk", "4", "--noise", "--denoise-guided"])):
        assert os.listdir(run_cli(tmp_path, f"refused{k}", flags, status=2)) == []
    # the library, same scene, same HDRI as decoded from the file
    cam_args, objs, heur = scenes.material_test()
    env = io.load_hdr(tmp_path / "env.hdr")
    scene, cam = rayrs_amd.Scene(objs, 1e-6, 1e6, heur, env, device=0), rayrs_amd.Camera(*cam_args)
    film = rayrs_amd.Film(scene, cam, sample_chunk=4, max_bounces=50, seed=77)
    film.render(4), film.render(4)
    io.save_hdr(tmp_path / "want_guided.hdr", film.denoised_guided(levels=3))
    assert (extra / "material_test_guided.hdr").read_bytes() == (tmp_path / "want_guided.hdr").read_bytes()
    io.save_hdr(tmp_path / "want_default.hdr", film.denoised_guided())
    assert (only / "material_test_guided.hdr").read_bytes() == (tmp_path / "want_default.hdr").read_bytes()
    with np.errstate(over="ignore"):
        noise3 = np.repeat(film.noise()[..., None], 3, axis=2).astype(np.float32)
    io.save_hdr(tmp_path / "want_noise.hdr", noise3)
    assert (extra / "material_test_noise.hdr").read_bytes() == (tmp_path / "want_noise.hdr").read_bytes()
