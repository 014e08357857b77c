"""The feature-guided a-trous filter on the GPU (include/rayrs_hip.h DENOISER), held bit for bit to the plain-Python
reference of tests/_features.py, whose exp is the oracle's: rayrs_image_denoise on seeded random frames with NaN and
infinite pixels, every level count up to steps beyond the image, every k switched off and every plane absent in turn;
a film's denoised frame against the reference applied to the film's frame and the oracle's features; the f32 format; the
command line's extra files."""
import os
import subprocess

import numpy as np
import pytest

import _features as F
import _film
import rayrs_amd
from rayrs_amd import _ffi, api, io, procedural, scenes

pytestmark = pytest.mark.gpu

SEED, BOUNCES, C = _film.SEED, _film.BOUNCES, _film.C
CLI = os.path.join(os.path.dirname(os.path.abspath(rayrs_amd.__file__)), "rayrs")
K = (4.0, 25.0, 0.3, 0.8)   # kn, ka, kz, kc
SIGMAS = dict(sigma_normal=0.5, sigma_albedo=0.2, sigma_depth=2.0, sigma_color=0.7)


def gpu_denoise(color, normal, albedo, depth, levels, kn, ka, kz, kc):
    """rayrs_image_denoise with the k themselves (rayrs_amd.denoise takes sigmas: 1 / sigma^2 need not give the k back)."""
    L = _ffi.lib()
    color = np.ascontiguousarray(color, dtype=np.float64)
    h, w = color.shape[:2]
    out = np.full((h, w, 3), 7.0)
    keep = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (normal, albedo, depth)]
    ptr = [None if a is None else a.ctypes.data for a in keep]
    _ffi.check(L.rayrs_image_denoise(0, w, h, color.ctypes.data, ptr[0], ptr[1], ptr[2], levels, kn, ka, kz, kc,
                                               out.ctypes.data), "rayrs_image_denoise")
    return out


def assert_same_frame(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if not F.same_bits(got, want):
        bad = (got.view(np.uint64) != want.view(np.uint64)).any(axis=2)
        y, x = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} pixels differ; first at ({y}, {x}): {got[y, x]} != {want[y, x]}")


@pytest.mark.parametrize("size", [(1, 1), (7, 5), (33, 17), (64, 48)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_filter_equals_the_reference_at_every_level_count(size):
    w, h = size
    color, normal, albedo, depth = F.random_case(100 + w, w, h)
    if w * h >= 8:
        assert not np.isfinite(color).all() and np.isnan(normal).any()
    for levels, want in enumerate(F.atrous_levels(color, normal, albedo, depth, 6, *K), start=1):   # step 32 at the last
        assert_same_frame(gpu_denoise(color, normal, albedo, depth, levels, *K), want, (size, levels))
    # the Python entry point with sigmas whose k are exact
    got = rayrs_amd.denoise(color, normal, albedo, depth, levels=2, sigma_normal=0.5, sigma_albedo=0.25, sigma_depth=2.0, sigma_color=1.0)
    assert_same_frame(got, F.atrous(color, normal, albedo, depth, 2, 4.0, 16.0, 0.25, 1.0), (size, "sigmas"))


def test_each_k_switched_off_and_each_plane_absent_in_turn():
    w, h = 33, 17
    color, normal, albedo, depth = F.random_case(5, w, h)
    for i in range(4):
        k = list(K)
        k[i] = 0.0
        assert_same_frame(gpu_denoise(color, normal, albedo, depth, 3, *k), F.atrous(color, normal, albedo, depth, 3, *k), ("k", i))
    planes = [normal, albedo, depth]
    for i in range(3):
        p = list(planes)
        p[i] = None
        assert_same_frame(gpu_denoise(color, *p, 3, *K), F.atrous(color, *p, 3, *K), ("plane", i))
    assert_same_frame(gpu_denoise(color, None, None, None, 3, *K), F.atrous(color, None, None, None, 3, *K), "no plane")
    # None and inf sigmas are k = 0
    got = rayrs_amd.denoise(color, normal, albedo, depth, levels=2, sigma_normal=None, sigma_albedo=float("inf"), sigma_depth=None,
                            sigma_color=0.5)
    assert_same_frame(got, F.atrous(color, normal, albedo, depth, 2, 0.0, 0.0, 0.0, 4.0), "sigmas off")


@pytest.mark.parametrize("name", ["sphere", "mesh"])
def test_a_films_denoised_frame_equals_the_reference(name):
    cam_args, objs, heur, env = _film.DESCS[name]()
    scene, cam = rayrs_amd.Scene(objs, 1e-6, 1e6, heur, env, device=0), rayrs_amd.Camera(*cam_args)
    film = rayrs_amd.Film(scene, cam, sample_chunk=C, max_bounces=BOUNCES, seed=SEED)
    feats = F.features_from(F.named_samples(name, 16), 16)
    k = [F.k_of(SIGMAS[s]) for s in ("sigma_normal", "sigma_albedo", "sigma_depth", "sigma_color")]

    def check(when, levels):
        frame = film.image(out_f64=True)
        want = F.atrous(frame, feats["normal"], feats["albedo"], feats["depth"], levels, *k)
        got = film.denoised(levels=levels, feature_samples=16, out_f64=True, **SIGMAS)
        assert_same_frame(got, want, (name, when))
        assert not F.same_bits(got, frame)                      # it did filter
        got32 = film.denoised(levels=levels, feature_samples=16, **SIGMAS)
        assert got32.dtype == np.float32 and F.same_bits(got32, want.astype(np.float32)), (name, when, "f32")
        assert F.same_bits(film.image(out_f64=True), frame)     # and left the film alone

    film.render(16)
    check("uniform", 5)
    # (the oracle's replay, tests/_film_adaptive.py: at tau 0.6 this pass takes 4 of the sphere's 12 tiles and 8 of the mesh's)
    active, _ = film.render_adaptive(4, 0.6, 24)
    per_tile = film.tile_samples()
    assert 0 < active < per_tile.size and len(np.unique(per_tile)) > 1, "the adaptive pass left every tile alike: pick another tau"
    check("tiles differ", 3)
    # the defaults run: a fraction of the scene's root-box diagonal for depth, the SIGMA_* starting points
    assert film.denoised().shape == (cam.y_pixels(), cam.x_pixels(), 3)


def run_cli(tmp, sub, args):
    d = tmp / sub
    d.mkdir()
    r = subprocess.run([CLI, str(tmp / "env.hdr"), "8", "--seed", "77"] + args, cwd=d, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return d


EXTRA = ["material_test_denoised.png", "material_test_denoised.hdr", "material_test_normal.png", "material_test_albedo.png",
         "material_test_depth.hdr"]


@pytest.mark.parametrize("mode", [[], ["--sample-chunk", "4", "--pass", "4"]], ids=["plain", "film"])
def test_the_command_line_writes_the_extra_files_and_the_same_ordinary_ones(tmp_path, mode):
    io.save_hdr(tmp_path / "env.hdr", procedural.make_hdri(128, 64))
    plain = run_cli(tmp_path, "without", mode)
    extra = run_cli(tmp_path, "with", mode + ["--denoise", "3", "--features"])
    for name in ("material_test.png", "material_test.hdr"):
        assert (plain / name).read_bytes() == (extra / name).read_bytes(), name
    assert sorted(os.listdir(plain)) == ["material_test.hdr", "material_test.png"]
    assert sorted(os.listdir(extra)) == sorted(EXTRA + ["material_test.hdr", "material_test.png"])
    for name in EXTRA:
        assert (extra / name).stat().st_size > 64, name
    # --denoise without a level count, as the last option and before another one
    last = run_cli(tmp_path, "last", mode + ["--denoise"])
    assert (last / "material_test_denoised.hdr").exists() and not (last / "material_test_normal.png").exists()
    mid = run_cli(tmp_path, "mid", ["--denoise", "--scene", "material_test"] + mode)
    assert (mid / "material_test_denoised.hdr").read_bytes() == (last / "material_test_denoised.hdr").read_bytes()
    # the library, same scene, same HDRI as decoded from the file
    cam_args, objs, heur = scenes.material_test()
    env = io.load_hdr(tmp_path / "env.hdr")
    scene, cam = rayrs_amd.Scene(objs, 1e-6, 1e6, heur, env, device=0), rayrs_amd.Camera(*cam_args)
    if mode:
        film = rayrs_amd.Film(scene, cam, sample_chunk=4, max_bounces=50, seed=77)
        film.render(4), film.render(4)
        want = film.denoised(levels=3)
        feats = film.features(16)
    else:
        frame, _ = rayrs_amd.render(scene, cam, 8, 50, seed=77, out_f64=True)
        feats = rayrs_amd.render_features(scene, cam, samples=16, seed=77)
        want = rayrs_amd.denoise(frame, feats["normal"], feats["albedo"], feats["depth"], levels=3,
                                 sigma_depth=api.scene_sigma_depth(scene)).astype(np.float32)
    io.save_hdr(tmp_path / "want.hdr", want)
    assert (extra / "material_test_denoised.hdr").read_bytes() == (tmp_path / "want.hdr").read_bytes()
    assert np.array_equal(io.load_hdr(extra / "material_test_denoised.hdr"), io.load_hdr(tmp_path / "want.hdr"))
    depth3 = np.repeat(feats["depth"][..., None], 3, axis=2).astype(np.float32)
    io.save_hdr(tmp_path / "depth.hdr", depth3)
    assert (extra / "material_test_depth.hdr").read_bytes() == (tmp_path / "depth.hdr").read_bytes()
