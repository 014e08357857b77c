"""Adaptive film passes (include/rayrs_hip.h rayrs_film_render_adaptive, rayrs_film_tile_samples) without a GPU: the
boundary's declarations, what is refused before the device is touched, item_geometry through a tile list, render_until's
adaptive stopping logic on a stub film, and the soundness and non-triviality of the oracle-side replay
(tests/_film_adaptive.py) that the GPU tests compare against."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import _film
import _film_adaptive as A
import rayrs_amd
from rayrs_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["rayrs_film_render_adaptive", "rayrs_film_tile_samples"]


def header():
    return open(os.path.join(ROOT, "include", "rayrs_hip.h")).read()


def test_the_header_declares_the_two_entry_points_and_the_library_exports_them():
    L = _ffi.lib()
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", code), name
        assert name in _ffi.SYMBOLS and hasattr(L, name), name
    assert L.rayrs_abi_version() == _ffi.ABI_VERSION == 7      # entry points were added, no struct or call changed
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"fn {name}\(", text), name


def test_the_header_states_the_contract_per_tile_and_the_selection_rule():
    text = re.sub(r"\s*\n \*\s*", " ", header())
    assert "ADAPTIVE PASSES" in text and "THE CONTRACT PER TILE" in text
    assert "the pixels rayrs_render returns for spp = N_t, sample_chunk = c" in text
    assert "N_t + n <= max_tile_samples" in text and "M = M_t = N_t / c" in text
    assert "in ascending tile order" in text
    assert "rayrs_film_status.samples is the largest N_t" in text


def test_refused_before_the_device_is_touched():
    L = _ffi.lib()
    st, active = _ffi.RenderStats(), C.c_uint64(7)
    call = lambda film, n, tau: L.rayrs_film_render_adaptive(film, n, tau, 0, C.byref(active), C.byref(st))
    assert call(None, 8, 0.5) == -1                      # a null film
    assert call(None, 0, 0.5) == -1                      # n = 0 is refused whatever the film
    assert call(None, 6, 0.5) == -1
    for tau in (-0.1, float("nan"), float("inf"), -float("inf")):
        assert call(None, 8, tau) == -1
    assert active.value == 7                             # nothing was written
    out = (C.c_uint32 * 4)()
    assert L.rayrs_film_tile_samples(None, out, 4) == 0
    # a film cannot exist on a host-only scene, so the rules on n % c and tau that need a film are in the GPU tests
    cam_args, objs, heur, env = _film.sphere_desc()
    scene = rayrs_amd.Scene(objs, 1e-6, 1e6, heur, env, device=-1)
    with pytest.raises(_ffi.RayrsError) as e:
        rayrs_amd.Film(scene, rayrs_amd.Camera(*cam_args))
    assert e.value.status == -4


SHIM = r"""
#include "layout.h"
extern "C" void item_window(unsigned spp, unsigned chunk, unsigned sample0, unsigned tile_rank, unsigned tile_ranks,
                            unsigned tiles_x, unsigned n_list, const unsigned* list, unsigned item, unsigned* out) {
    rayrs::RenderDev rp = {};
    rp.spp = spp, rp.chunk = chunk, rp.sample0 = sample0;
    rp.nchunks = (spp + chunk - 1) / chunk;
    rp.tile_rank = tile_rank, rp.tile_ranks = tile_ranks, rp.tiles_x = tiles_x;
    rp.inv_nchunks = 1.0 / (double)rp.nchunks, rp.inv_tiles_x = 1.0 / (double)tiles_x;
    if (list) rp.tile_list = reinterpret_cast<const rayrs::TileRef*>(list), rp.n_local_tiles = n_list;
    rayrs::item_geometry(rp, item, out[0], out[1], out[2], out[3]);
}
"""


def test_item_geometry_through_a_tile_list(tmp_path):
    """layout.h item_geometry compiled for the host: with a list, local tile lt is list[lt].tile and its window begins at
    list[lt].samples instead of sample0; a null list gives the share's mapping and sample0."""
    cxx = shutil.which("g++") or shutil.which("c++") or "/opt/rocm/bin/hipcc"
    src = tmp_path / "shim.cpp"
    src.write_text(SHIM)
    lib = tmp_path / "libshim.so"
    cmd = [cxx] + (["-x", "c++"] if cxx.endswith("hipcc") else []) + ["-std=c++17", "-O1", "-shared", "-fPIC", "-ffp-contract=off",
           "-I", os.path.join(ROOT, "rayrs_amd", "csrc"), "-o", str(lib), str(src)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    fn = C.CDLL(str(lib)).item_window
    fn.argtypes = [C.c_uint32] * 7 + [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    fn.restype = None
    rng = np.random.default_rng(11)
    out = (C.c_uint32 * 4)()
    for _ in range(2000):
        c = int(rng.integers(1, 9))
        spp = int(rng.integers(1, 9)) * c
        ranks = int(rng.integers(1, 5))
        rank = int(rng.integers(0, ranks))
        tiles_x = int(rng.integers(1, 40))
        sample0 = int(rng.integers(0, 1 << 20)) * c
        nchunks = spp // c
        n_list = int(rng.integers(1, 50))
        tiles = np.sort(rng.choice(4000, size=n_list, replace=False)).astype(np.uint32)
        counts = (rng.integers(0, 1 << 20, size=n_list) * c).astype(np.uint32)
        pairs = np.ascontiguousarray(np.stack([tiles, counts], axis=1))    # (tile, N_t), 8 bytes each
        item = int(rng.integers(0, 64 * nchunks * n_list))
        fn(spp, c, sample0, rank, ranks, tiles_x, n_list, pairs.ctypes.data, item, out)
        # the three-line restatement
        lt, chunk = (item >> 6) // nchunks, (item >> 6) % nchunks
        tile, s_begin = int(tiles[lt]), int(counts[lt]) + chunk * c
        assert (out[2], out[3]) == (s_begin, min(s_begin + c, int(counts[lt]) + spp)), (spp, c, item)
        assert (out[0], out[1]) == ((tile // tiles_x) * 8 + ((item & 63) >> 3), (tile % tiles_x) * 8 + (item & 7))
        # a null list: today's answer
        fn(spp, c, sample0, rank, ranks, tiles_x, 0, None, item, out)
        tile, s_begin = lt * ranks + rank, sample0 + chunk * c
        assert (out[2], out[3]) == (s_begin, min(s_begin + c, sample0 + spp))
        assert (out[0], out[1]) == ((tile // tiles_x) * 8 + ((item & 63) >> 3), (tile % tiles_x) * 8 + (item & 7))


class StubCamera:
    def x_pixels(self):
        return 32

    def y_pixels(self):
        return 24


class StubFilm:
    """What render_until(adaptive=True) sees of a film: per pass, the tiles that are still noisy get the step, up to the cap."""

    def __init__(self, noisy_for, c=4):
        self.sample_chunk, self.tile_rank, self.tile_ranks, self.camera = c, 0, 1, StubCamera()
        self.noisy_for = np.asarray(noisy_for, dtype=np.uint32)    # a tile is noisy while it holds fewer samples than this
        self.nt = np.zeros_like(self.noisy_for)
        self.calls = []

    def pixels(self):
        return 32 * 24

    def render(self, n):
        raise AssertionError("an adaptive render_until adds no uniform pass")

    def render_adaptive(self, n, tau, max_tile_samples=0):
        assert n > 0 and n % self.sample_chunk == 0
        take = (self.nt < self.noisy_for) & (self.nt + n <= (max_tile_samples or 1 << 30))
        self.nt[take] += n
        self.calls.append((n, tau, max_tile_samples, int(take.sum())))
        return int(take.sum()), {"rays": 10 * n * int(take.sum()), "paths": n * int(take.sum())}

    def tile_samples(self):
        return self.nt.copy()

    def sample_map(self):
        return np.repeat(np.repeat(self.nt, 8, axis=0), 8, axis=1)

    def status(self, tau):
        n = int(self.nt.max())
        return dict(samples=n, full_chunks=n // self.sample_chunk, rays=0, paths=0, nan_pixels=0, neg_pixels=0,
                    unconverged=64 * int((self.nt < self.noisy_for).sum()), nonfinite=0, closed=0)


def test_render_until_adaptive_on_a_stub_film():
    noisy_for = np.array([[8, 8, 16, 8], [24, 8, 8, 8], [8, 40, 8, 16]])
    f = StubFilm(noisy_for)
    seen = []
    st, why = rayrs_amd.render_until(f, 0.5, 0.0, pass_samples=8, max_samples=64, adaptive=True,
                                     on_pass=lambda film, s: seen.append((s["active_tiles"], s["unconverged"])))
    assert why == "converged" and [c[3] for c in f.calls] == [12, 4, 2, 1, 1]
    assert all(c[:3] == (8, 0.5, 64) for c in f.calls)
    assert seen == [(12, 4 * 64), (4, 2 * 64), (2, 64), (1, 64), (1, 0)]
    assert np.array_equal(f.nt, noisy_for)
    assert (st["tile_samples_min"], st["tile_samples_max"], st["samples"]) == (8, 40, 40)
    assert st["pixel_samples"] == 64 * int(noisy_for.sum()) and st["pixels"] == 768 and st["unconverged"] == 0
    # the cap: a pass that selects no tile while pixels are still unconverged
    f = StubFilm(noisy_for)
    st, why = rayrs_amd.render_until(f, 0.5, 0.0, pass_samples=8, max_samples=20, adaptive=True)
    assert why == "max_samples" and [c[3] for c in f.calls] == [12, 4, 0]
    assert st["tile_samples_max"] == 16 and st["unconverged"] == 2 * 64
    assert np.array_equal(f.nt, np.minimum(noisy_for, 16))
    # pass_samples is rounded up to whole chunks; a cap below one pass adds none
    f = StubFilm(np.full((3, 4), 12))
    st, why = rayrs_amd.render_until(f, 0.5, 0.0, pass_samples=9, max_samples=64, adaptive=True)
    assert why == "converged" and [c[0] for c in f.calls] == [12]
    f = StubFilm(noisy_for)
    st, why = rayrs_amd.render_until(f, 0.5, 0.0, pass_samples=8, max_samples=4, adaptive=True)
    assert why == "max_samples" and f.calls == []
    # a fraction, the time budget, a film that is already converged
    f = StubFilm(noisy_for)
    st, why = rayrs_amd.render_until(f, 0.5, 0.2, pass_samples=8, max_samples=64, adaptive=True)
    assert why == "converged" and [c[3] for c in f.calls] == [12, 4]      # 2 * 64 of 768 is 16.7 %
    f = StubFilm(noisy_for)
    st, why = rayrs_amd.render_until(f, 0.5, 0.0, pass_samples=8, max_samples=64, adaptive=True, time_budget_s=0.0)
    assert why == "time_budget" and f.calls == []
    f = StubFilm(noisy_for)
    f.nt[:] = noisy_for
    st, why = rayrs_amd.render_until(f, 0.5, 0.0, pass_samples=8, max_samples=64, adaptive=True)
    assert why == "converged" and f.calls == []


@pytest.mark.parametrize("name", ["sphere", "mesh"])
def test_the_replay_is_sound_and_not_trivial(name):
    """The replay stands on the oracle: the per-sample iteration counts add up to orc_render's rays for every sample count
    in use, a uniform replay is _film.expectation exactly; and the stated settings exercise the rule: a pass selects a
    proper, non-empty subset of the tiles, at least three distinct N_t remain, sphere converges below the cap, mesh stops
    on it."""
    rgb, it = A.named_traces(name)
    assert rgb.shape == (A.H, A.W, A.CAP, 3) and it.shape == (A.H, A.W, A.CAP)
    rep = A.Replay(rgb, it)
    passes, why = A.replay_until(rep)
    n_tiles = rep.ty * rep.tx
    per_pass = [p["active_tiles"] for p in passes]
    finals = sorted(set(int(v) for v in rep.nt.ravel()))
    print(f"{name}: active tiles per pass {per_pass}, {why}; tile-samples {sum(per_pass) * A.PASS} of {n_tiles * int(rep.nt.max())} "
          f"uniform; final counts {finals}")
    assert per_pass[0] == n_tiles                                  # an empty film: every tile
    assert any(0 < a < n_tiles for a in per_pass)
    assert len(finals) >= 3
    assert all(p["nonfinite"] == 0 for p in passes)
    if name == "sphere":
        assert why == "converged" and rep.nt.max() < A.CAP and passes[-1]["unconverged"] == 0
    else:
        assert why == "max_samples" and rep.nt.max() == A.CAP and passes[-1]["unconverged"] > 0
    assert sum(p["paths"] for p in passes) == rep.pixel_samples()
    # a tile's N_t only ever grows by whole passes, and an inactive tile's pixels do not move
    for before, after in zip(passes, passes[1:]):
        grown = after["nt"] != before["nt"]
        assert np.array_equal(grown, after["active"]) and np.array_equal(after["nt"][grown], before["nt"][grown] + A.PASS)
        still = ~np.repeat(np.repeat(grown, 8, axis=0), 8, axis=1)
        assert np.array_equal(after["frame"][still].view(np.uint64), before["frame"][still].view(np.uint64))
    # the sum of n is the oracle's ray count, and the frame at N the oracle's, for every N in use
    osc, ocam = _film.oracle_of(_film.DESCS[name](A.W, A.H))
    for n in finals:
        ref, ost = osc.render(ocam, n, A.BOUNCES, A.SEED, sample_chunk=A.C)
        assert int(it[:, :, :n].sum()) == ost["rays"] and A.W * A.H * n == ost["paths"], (name, n)
        assert np.array_equal(rep.at(n)[0].view(np.uint64), ref.view(np.uint64)), (name, n)
    # a uniform replay is _film.expectation
    uni = A.Replay(rgb, it)
    rays = 0
    for k in (8, 16, 6):
        p = uni.uniform_pass(k)
        rays += p["rays"]
        n = int(uni.nt.max())
        frame, s1, s2, m = _film.expectation(rgb, A.C, n)
        assert (uni.nt == n).all() and p["active_tiles"] == n_tiles
        assert np.array_equal(p["frame"].view(np.uint64), frame.view(np.uint64))
        assert np.array_equal(p["s1"].view(np.uint64), s1.view(np.uint64)) and np.array_equal(p["s2"].view(np.uint64), s2.view(np.uint64))
        assert (p["unconverged"], p["nonfinite"]) == _film.noise_counts(s1, s2, m, A.TAU)
        assert rays == int(it[:, :, :n].sum())
    assert uni.closed
