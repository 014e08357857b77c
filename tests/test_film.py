"""The progressive film (include/rayrs_hip.h rayrs_film_*) without a GPU: the boundary's declarations and layouts,
every rule that can be refused before the device is touched, render_until's stopping logic on a stub film, the sample
window in item_geometry, and the soundness of the oracle-side reconstruction the GPU tests compare against."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import _film
import rayrs_amd
from rayrs_amd import _ffi, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILM_SYMBOLS = ["rayrs_film_create", "rayrs_film_destroy", "rayrs_film_render", "rayrs_film_read", "rayrs_film_status_get",
                "rayrs_film_state_bytes", "rayrs_film_state_get", "rayrs_film_state_set"]


def header():
    return open(os.path.join(ROOT, "include", "rayrs_hip.h")).read()


def test_the_header_declares_the_film_and_the_library_exports_it():
    L = _ffi.lib()
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in FILM_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", code), name
        assert name in _ffi.SYMBOLS and hasattr(L, name), name
    assert "typedef struct rayrs_film rayrs_film;" in code
    assert L.rayrs_abi_version() == _ffi.ABI_VERSION == 7


def test_the_header_states_the_definition_and_the_rules():
    text = re.sub(r"\s*\n \*\s*", " ", header())
    assert "M*S2 - S1*S1 <= ((tau*tau) * (S1*S1)) * (M-1)" in text
    assert "BATCH-MEANS" in text and "NOT a per-sample variance" in text
    assert "rayrs_render_multi does not take films" in text
    assert "Destroying the scene before its films is the caller's error" in text
    assert "one pass or one plain render in flight per scene" in text


def layout_table():
    L = _ffi.lib()
    n = L.rayrs_abi_layout(None, 0)
    table = (C.c_uint32 * n)()
    assert L.rayrs_abi_layout(table, n) == n
    return list(table)


def test_the_two_structs_end_the_layout_table_with_the_ctypes_offsets():
    table = layout_table()
    assert _ffi.ABI_STRUCTS[-3:] == [_ffi.Tuning, _ffi.FilmParams, _ffi.FilmStatus]
    tail = []
    for st in (_ffi.FilmParams, _ffi.FilmStatus):
        tail += [C.sizeof(st), len(st._fields_)] + [getattr(st, name).offset for name, _ in st._fields_]
    assert table[-len(tail):] == tail
    assert [n for n, _ in _ffi.FilmParams._fields_] == ["sample_chunk", "max_bounces", "seed", "tile_rank", "tile_ranks",
                                                        "fast_traversal", "pad"]
    assert [n for n, _ in _ffi.FilmStatus._fields_] == ["samples", "full_chunks", "rays", "paths", "nan_pixels", "neg_pixels",
                                                        "unconverged", "nonfinite", "closed", "pad"]
    assert C.sizeof(_ffi.FilmParams) == 32 and C.sizeof(_ffi.FilmStatus) == 72


def test_integration_md_quotes_the_film_structs():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for st, cname in ((_ffi.FilmParams, "rayrs_film_params"), (_ffi.FilmStatus, "rayrs_film_status")):
        assert re.search(rf"{cname}\W+{C.sizeof(st)} bytes", text), f"INTEGRATION.md: {cname} is {C.sizeof(st)} bytes"
    for name in FILM_SYMBOLS:
        assert re.search(rf"fn {name}\(", text), name


def host_scene_and_camera():
    cam_args, objs, heur, env = _film.sphere_desc()
    return rayrs_amd.Scene(objs, 1e-6, 1e6, heur, env, device=-1), rayrs_amd.Camera(*cam_args)


def create(scene, cam, **kw):
    L = _ffi.lib()
    p = _ffi.FilmParams()
    for k, v in kw.items():
        setattr(p, k, v)
    h = C.c_void_p()
    st = L.rayrs_film_create(scene._h if scene else None, C.byref(cam.desc) if cam else None, C.byref(p), C.byref(h))
    return st, h


def test_rules_refused_before_the_device_is_touched():
    L = _ffi.lib()
    scene, cam = host_scene_and_camera()
    p, h = _ffi.FilmParams(), C.c_void_p()
    # null pointers
    assert L.rayrs_film_create(None, C.byref(cam.desc), C.byref(p), C.byref(h)) == -1
    assert L.rayrs_film_create(scene._h, None, C.byref(p), C.byref(h)) == -1
    assert L.rayrs_film_create(scene._h, C.byref(cam.desc), None, C.byref(h)) == -1
    assert L.rayrs_film_create(scene._h, C.byref(cam.desc), C.byref(p), None) == -1
    st = _ffi.RenderStats()
    fs = _ffi.FilmStatus()
    buf = (C.c_uint8 * 128)()
    assert L.rayrs_film_render(None, 4, C.byref(st)) == -1
    assert L.rayrs_film_render(None, 0, C.byref(st)) == -1          # n = 0 is refused whatever the film
    assert L.rayrs_film_read(None, 1, buf) == -1
    assert L.rayrs_film_status_get(None, 0.2, C.byref(fs)) == -1
    assert L.rayrs_film_state_bytes(None) == 0
    assert L.rayrs_film_state_get(None, buf, 128) == -1
    assert L.rayrs_film_state_set(None, buf, 128) == -1
    L.rayrs_film_destroy(None)
    # a film on a host-only scene: settings are validated first, then RAYRS_NO_DEVICE
    assert create(scene, cam)[0] == -4
    assert create(scene, cam, sample_chunk=4, max_bounces=50, tile_rank=0, tile_ranks=1)[0] == -4
    assert create(scene, cam, sample_chunk=1 << 30)[0] == -5          # no full chunk fits the 30-bit sample cursor
    assert create(scene, cam, sample_chunk=(1 << 30) - 1)[0] == -4
    assert create(scene, cam, max_bounces=8001)[0] == -5
    assert create(scene, cam, tile_rank=3, tile_ranks=3)[0] == -1
    assert create(scene, cam, tile_rank=1, tile_ranks=0)[0] == -1
    assert create(scene, cam, fast_traversal=2)[0] == -1
    assert create(scene, cam, pad=1)[0] == -1
    big = rayrs_amd.Camera(*scenes.camera_for_resolution(_film.sphere_desc()[0], 70000, 8))
    assert create(scene, big)[0] == -5                               # today's limit on an image side
    with pytest.raises(_ffi.RayrsError) as e:
        rayrs_amd.Film(scene, cam)
    assert e.value.status == -4


class StubFilm:
    """Replays statuses: what render_until sees of a film."""

    def __init__(self, unconverged_after, c=4, pixels=768, closes_at=None):
        self.sample_chunk, self._pixels, self.after, self.closes_at = c, pixels, unconverged_after, closes_at
        self.samples, self.passes = 0, []

    def pixels(self):
        return self._pixels

    def render(self, n):
        assert n > 0 and not self.status(0)["closed"]
        self.passes.append(n)
        self.samples += n
        return {"rays": 10 * n, "paths": n}

    def status(self, tau):
        unc = self._pixels if self.samples == 0 else self.after.get(self.samples, 0)
        return dict(samples=self.samples, full_chunks=self.samples // self.sample_chunk, rays=0, paths=0, nan_pixels=0,
                    neg_pixels=0, unconverged=unc, nonfinite=0, closed=int(self.closes_at is not None and self.samples >= self.closes_at))


def test_render_until_stops_where_the_statuses_say():
    after = {8: 130, 16: 16, 24: 1, 32: 0, 40: 0}
    f = StubFilm(after)
    seen = []
    st, why = rayrs_amd.render_until(f, 0.5, 0.0, pass_samples=8, max_samples=64, on_pass=lambda film, s: seen.append(s["samples"]))
    assert why == "converged" and st["samples"] == 32 and f.passes == [8, 8, 8, 8] and seen == [8, 16, 24, 32]
    assert st["pixels"] == 768 and st["unconverged"] == 0
    # a fraction: 16 of 768 is 2.08 %
    f = StubFilm(after)
    st, why = rayrs_amd.render_until(f, 0.5, 0.03, pass_samples=8, max_samples=64)
    assert why == "converged" and st["samples"] == 16
    # the sample budget: never beyond max_samples, and it says so
    f = StubFilm(after)
    st, why = rayrs_amd.render_until(f, 0.5, 0.0, pass_samples=8, max_samples=8)
    assert why == "max_samples" and st["samples"] == 8 and f.passes == [8]
    f = StubFilm(after)
    st, why = rayrs_amd.render_until(f, 0.5, 0.0, pass_samples=8, max_samples=20)
    assert why == "max_samples" and st["samples"] == 16
    # pass_samples is rounded up to whole chunks
    f = StubFilm({12: 5, 24: 0}, c=4)
    st, why = rayrs_amd.render_until(f, 0.5, 0.0, pass_samples=9, max_samples=64)
    assert f.passes == [12, 12] and why == "converged"
    # the time budget: checked before each pass
    f = StubFilm(after)
    st, why = rayrs_amd.render_until(f, 0.5, 0.0, pass_samples=8, max_samples=64, time_budget_s=0.0)
    assert why == "time_budget" and f.passes == []
    # a film that is already converged gets no pass; an empty one is never "converged"
    f = StubFilm({8: 0})
    f.samples = 8
    st, why = rayrs_amd.render_until(f, 0.5, 0.0, pass_samples=8, max_samples=64)
    assert why == "converged" and f.passes == []
    with pytest.raises(ValueError):
        rayrs_amd.render_until(StubFilm(after), 0.5, pass_samples=0)


SHIM = r"""
#include "layout.h"
extern "C" void item_window(unsigned spp, unsigned chunk, unsigned sample0, unsigned tile_rank, unsigned tile_ranks,
                            unsigned tiles_x, unsigned item, unsigned* out) {
    rayrs::RenderDev rp = {};
    rp.spp = spp, rp.chunk = chunk, rp.sample0 = sample0;
    rp.nchunks = (spp + chunk - 1) / chunk;
    rp.tile_rank = tile_rank, rp.tile_ranks = tile_ranks, rp.tiles_x = tiles_x;
    rp.inv_nchunks = 1.0 / (double)rp.nchunks, rp.inv_tiles_x = 1.0 / (double)tiles_x;
    rayrs::item_geometry(rp, item, out[0], out[1], out[2], out[3]);
}
"""


def test_item_geometry_with_a_window_start(tmp_path):
    """layout.h item_geometry compiled for the host (RR_LAYOUT_FN): an item's samples are sample0 + chunk * c .. clamped
    to the window's end sample0 + spp, and its pixel does not depend on the window."""
    cxx = shutil.which("g++") or shutil.which("c++") or "/opt/rocm/bin/hipcc"
    src = tmp_path / "shim.cpp"
    src.write_text(SHIM)
    lib = tmp_path / "libshim.so"
    cmd = [cxx] + (["-x", "c++"] if cxx.endswith("hipcc") else []) + ["-std=c++17", "-O1", "-shared", "-fPIC", "-ffp-contract=off",
           "-I", os.path.join(ROOT, "rayrs_amd", "csrc"), "-o", str(lib), str(src)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    fn = C.CDLL(str(lib)).item_window
    fn.argtypes = [C.c_uint32] * 7 + [C.POINTER(C.c_uint32)]
    fn.restype = None
    rng = np.random.default_rng(7)
    out = (C.c_uint32 * 4)()
    for _ in range(2000):
        c = int(rng.integers(1, 9))
        spp = int(rng.integers(1, 70))           # (spp % c != 0: the window ends in a short chunk)
        sample0 = int(rng.integers(0, 1 << 20)) * c if rng.integers(0, 4) else 0
        ranks = int(rng.integers(1, 5))
        rank = int(rng.integers(0, ranks))
        tiles_x = int(rng.integers(1, 40))
        nchunks = -(-spp // c)
        item = int(rng.integers(0, 64 * nchunks * 50))
        fn(spp, c, sample0, rank, ranks, tiles_x, item, out)
        # the three-line restatement
        chunk = (item >> 6) % nchunks
        s_begin = sample0 + chunk * c
        s_end = min(s_begin + c, sample0 + spp)
        tile = ((item >> 6) // nchunks) * ranks + rank
        assert (out[2], out[3]) == (s_begin, s_end), (spp, c, sample0, item)
        assert (out[0], out[1]) == ((tile // tiles_x) * 8 + ((item & 63) >> 3), (tile % tiles_x) * 8 + (item & 7))
    # the last sample index a film can reach
    fn(4, 4, (1 << 30) - 8, 0, 1, 1, 0, out)
    assert (out[2], out[3]) == ((1 << 30) - 8, (1 << 30) - 4)


SHARE_SHIM = r"""
#include "layout.h"
// out: (tile, row, col, in_share) of every lane of the local tiles 0 .. n_local_tiles + 1; share: the five fields
extern "C" void share_pixels(unsigned x_pixels, unsigned y_pixels, unsigned rank, unsigned ranks, unsigned* share, unsigned* out) {
    const rayrs::TileShare ts = rayrs::tile_share(x_pixels, y_pixels, rank, ranks);
    share[0] = ts.tile_rank, share[1] = ts.tile_ranks, share[2] = ts.tiles_x, share[3] = ts.tiles_y, share[4] = ts.n_local_tiles;
    rayrs::RenderDev rp = {};   // the kernels that take a RenderDev map through share_of
    rp.tile_rank = ts.tile_rank, rp.tile_ranks = ts.tile_ranks, rp.tiles_x = ts.tiles_x, rp.tiles_y = ts.tiles_y;
    rp.n_local_tiles = ts.n_local_tiles;
    for (unsigned lt = 0; lt <= ts.n_local_tiles + 1; lt++)
        for (unsigned pit = 0; pit < 64; pit++) {
            const rayrs::TilePixel p = rayrs::tile_pixel(lt & 1 ? rayrs::share_of(rp) : ts, lt, pit);
            *out++ = p.tile, *out++ = p.row, *out++ = p.col, *out++ = p.in_share ? 1u : 0u;
        }
}
"""


def test_tile_share_and_tile_pixel_are_the_three_line_mapping(tmp_path):
    """layout.h tile_share, share_of and tile_pixel compiled for the host, exhaustively for frames up to 40 x 24 and up to
    seven ranks: the share's fields, every lane of every local tile and of the two local tiles past the share against the
    three-line restatement; the ranks' shares partition the frame's tiles, and their in-image pixels the image."""
    cxx = shutil.which("g++") or shutil.which("c++") or "/opt/rocm/bin/hipcc"
    src = tmp_path / "share_shim.cpp"
    src.write_text(SHARE_SHIM)
    lib = tmp_path / "libshare_shim.so"
    cmd = [cxx] + (["-x", "c++"] if cxx.endswith("hipcc") else []) + ["-std=c++17", "-O1", "-shared", "-fPIC", "-ffp-contract=off",
           "-I", os.path.join(ROOT, "rayrs_amd", "csrc"), "-o", str(lib), str(src)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    fn = C.CDLL(str(lib)).share_pixels
    fn.argtypes = [C.c_uint32] * 4 + [C.POINTER(C.c_uint32)] * 2
    fn.restype = None
    share = (C.c_uint32 * 5)()
    buf = np.zeros((15 + 2) * 64 * 4, dtype=np.uint32)   # 40 x 24 is 5 x 3 tiles
    out = buf.ctypes.data_as(C.POINTER(C.c_uint32))
    pit_of = np.tile(np.arange(64), 17)
    lt_of = np.repeat(np.arange(17), 64)
    for x in range(1, 41):
        for y in range(1, 25):
            tiles_x, tiles_y = (x + 7) // 8, (y + 7) // 8
            n_tiles = tiles_x * tiles_y
            for ranks in range(1, 8):
                owned, cover = [], np.zeros((y, x), dtype=np.int64)
                for rank in range(ranks):
                    fn(x, y, rank, ranks, share, out)
                    n_local = len(range(rank, n_tiles, ranks))
                    assert list(share) == [rank, ranks, tiles_x, tiles_y, n_local], (x, y, rank, ranks)
                    if rank >= n_tiles:
                        assert share[4] == 0   # more ranks than tiles: the surplus ranks own nothing
                    k = (n_local + 2) * 64
                    got = buf[:4 * k].reshape(k, 4).astype(np.int64)
                    lt, pit = lt_of[:k], pit_of[:k]
                    inside = lt < n_local
                    tile = np.where(inside, lt * ranks + rank, 0)   # the three-line restatement
                    row = (tile // tiles_x) * 8 + (pit >> 3)
                    col = (tile % tiles_x) * 8 + (pit & 7)
                    assert np.array_equal(got, np.stack([tile, row, col, inside.astype(np.int64)], axis=1)), (x, y, rank, ranks)
                    assert (got[~inside][:, 0] == 0).all() and (~inside).sum() == 128   # past the share: tile 0, not in it
                    owned += list(got[inside][::64, 0])
                    seen = inside & (row < y) & (col < x)
                    np.add.at(cover, (row[seen], col[seen]), 1)
                assert sorted(owned) == list(range(n_tiles)), (x, y, ranks)
                assert (cover == 1).all(), (x, y, ranks)


@pytest.mark.parametrize("name", ["sphere", "mesh"])
def test_the_oracle_side_reconstruction_is_sound(name):
    """The frame rebuilt from per-sample traces equals orc_render's bit for bit (so S1, S2 and the converged counts the
    GPU tests derive from the same traces stand on the oracle), and the predicate is not trivial on these scenes."""
    osc, ocam = _film.oracle_of(_film.DESCS[name]())
    rgb = _film.named_traces(name, 32)
    for n in (16, 32, 30):
        ref, _ = osc.render(ocam, n, _film.BOUNCES, _film.SEED, sample_chunk=_film.C)
        frame, s1, s2, m = _film.expectation(rgb, _film.C, n)
        assert m == n // _film.C
        assert np.array_equal(frame.view(np.uint64), ref.view(np.uint64)), (name, n)
        assert np.isfinite(s1).all() and np.isfinite(s2).all()
        unc, nonf = _film.noise_counts(s1, s2, m, 0.2)
        assert nonf == 0 and 0 < unc < _film.W * _film.H, (name, n, unc)
        assert _film.noise_counts(s1, s2, m, 0.05)[0] >= unc >= _film.noise_counts(s1, s2, m, 0.5)[0]
    assert _film.noise_counts(*_film.expectation(rgb, _film.C, 4)[1:], 0.5) == (_film.W * _film.H, 0)   # M = 1
