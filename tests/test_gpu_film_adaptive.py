"""Adaptive film passes on the GPU (include/rayrs_hip.h ADAPTIVE PASSES), held bit for bit to the replay of the selection
rule on the CPU oracle's per-sample traces (tests/_film_adaptive.py): after every pass the active tiles, the per-tile
sample counts, the frame in both formats, the noise counts with per-tile M and the pass's rays and paths; mixed
histories, checkpoints, tile shares, ragged images, non-finite pixels, the fast walk and the command line."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _film
import _film_adaptive as A
import _nonfinite as N
import _oracle
import rayrs_amd
from rayrs_amd import _ffi, io, procedural, scenes, tiles

pytestmark = pytest.mark.gpu

C, SEED, BOUNCES, W, H = A.C, A.SEED, A.BOUNCES, A.W, A.H
HERE = os.path.dirname(os.path.abspath(__file__))
CLI = os.path.join(os.path.dirname(os.path.abspath(rayrs_amd.__file__)), "rayrs")
# test_gpu_film.py's three: the local-pool route, the same scene on the streaming route, a mesh on the streaming route
VARIANTS = [("sphere", 0), ("sphere", 1), ("mesh", 0)]
IDS = ["sphere-local-pool", "sphere-streaming", "mesh-streaming"]


class Setup:
    def __init__(self, name, local_pool, w=W, h=H, samples=A.CAP):
        self.name, self.desc = name, _film.DESCS[name](w, h)
        cam_args, objs, heur, env = self.desc
        self.scene = rayrs_amd.Scene(objs, 1e-6, 1e6, heur, env, device=0)
        self.scene.set_tuning(local_pool=local_pool)
        assert self.scene.info()["local_pool"] == (1 if name == "sphere" and local_pool == 0 else 0)
        self.cam = rayrs_amd.Camera(*cam_args)
        self.osc, self.ocam = _film.oracle_of(self.desc)
        self.rgb, self.it = A.named_traces(name, samples, w, h)

    def film(self, **kw):
        kw.setdefault("sample_chunk", C)
        return rayrs_amd.Film(self.scene, self.cam, max_bounces=BOUNCES, seed=SEED, **kw)

    def replay(self, **kw):
        return A.Replay(self.rgb, self.it, C, **kw)


def same_bits(a, b, nan_aware=False):
    if nan_aware:
        N.assert_same_frame_nan_aware(a, b)
        return True
    ui = np.uint64 if a.dtype == np.float64 else np.uint32
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(ui), np.ascontiguousarray(b).view(ui))


def check_film(film, rep, what, nan_aware=False, taus=_film.TAUS):
    """The film as it stands against the replay as it stands: N_t, both frames, the counts at three taus."""
    assert np.array_equal(film.tile_samples(), rep.nt), what
    assert film.tile_samples().dtype == np.uint32 and film.sample_map().shape == (rep.h, rep.w)
    if rep.nt.max() == 0:
        return
    want = rep.frame()
    img = film.image(out_f64=True)
    assert same_bits(img, want, nan_aware), f"{what}: {int((img.view(np.uint64) != want.view(np.uint64)).any(axis=2).sum())} pixels differ"
    img32 = film.image()
    with np.errstate(all="ignore"):
        assert img32.dtype == np.float32 and same_bits(img32, want.astype(np.float32), nan_aware), what
    n_max = int(rep.nt.max())
    for tau in taus:
        st = film.status(tau)
        assert (st["unconverged"], st["nonfinite"]) == rep.counts(tau), (what, tau)
        assert (st["samples"], st["full_chunks"], st["closed"]) == (n_max, n_max // C, int(rep.closed)), what


def adaptive_pass(film, rep, n, tau, cap, what, nan_aware=False):
    """One pass on both sides; everything the pass reports and leaves is compared."""
    p = rep.adaptive_pass(n, tau, cap)
    active, st = film.render_adaptive(n, tau, cap)
    print(f"{what}: {active} active tiles (replay {p['active_tiles']}), rays {st['rays']} (replay {p['rays']})")
    assert active == p["active_tiles"], what
    assert (st["rays"], st["paths"]) == (p["rays"], p["paths"]), what
    check_film(film, rep, what, nan_aware)
    return p, st


@pytest.mark.parametrize("variant", VARIANTS, ids=IDS)
def test_every_adaptive_pass_is_the_replays(variant):
    s = Setup(*variant)
    film, rep = s.film(), s.replay()
    check_film(film, rep, "empty")
    rays = paths = 0
    per_pass = []
    for k in range(A.CAP // A.PASS + 1):
        p, st = adaptive_pass(film, rep, A.PASS, A.TAU, A.CAP, f"{variant} pass {k}")
        if p["active_tiles"]:
            assert st["local_pool"] == s.scene.info()["local_pool"]
        rays, paths = rays + st["rays"], paths + st["paths"]
        per_pass.append(p["active_tiles"])
        fs = film.status(A.TAU)
        assert (fs["rays"], fs["paths"]) == (rays, paths)
        if p["active_tiles"] == 0:
            break
    n_tiles = rep.ty * rep.tx
    assert per_pass[0] == n_tiles and per_pass[-1] == 0 and any(0 < a < n_tiles for a in per_pass), per_pass
    assert len(set(int(v) for v in rep.nt.ravel())) >= 3
    fs = film.status(A.TAU)
    assert (fs["unconverged"] == 0) == (s.name == "sphere")   # sphere converges below the cap, mesh stops on it
    assert paths == rep.pixel_samples()
    # every tile is the one-shot render at its own count: the oracle's frame, not only the traces'
    img = film.image(out_f64=True)
    for n in sorted(set(int(v) for v in rep.nt.ravel())):
        ref, _ = s.osc.render(s.ocam, n, BOUNCES, SEED, sample_chunk=C)
        mask = np.repeat(np.repeat(rep.nt == n, 8, axis=0), 8, axis=1)
        assert np.array_equal(img[mask].view(np.uint64), ref[mask].view(np.uint64)), (variant, n)


@pytest.mark.parametrize("variant", VARIANTS, ids=IDS)
def test_render_until_adaptive_stops_where_the_replay_says(variant):
    s = Setup(*variant)
    rep = s.replay()
    passes, why = A.replay_until(rep)
    film = s.film()
    seen = []
    st, reason = rayrs_amd.render_until(film, A.TAU, 0.0, pass_samples=A.PASS, max_samples=A.CAP, adaptive=True,
                                        on_pass=lambda f, x: seen.append((x["active_tiles"], x["unconverged"])))
    assert reason == why and seen == [(p["active_tiles"], p["unconverged"]) for p in passes]
    assert (st["tile_samples_min"], st["tile_samples_max"]) == (int(rep.nt.min()), int(rep.nt.max()))
    assert st["pixel_samples"] == rep.pixel_samples() and st["pixels"] == W * H
    check_film(film, rep, f"{variant} after render_until")


@pytest.mark.parametrize("variant", VARIANTS, ids=IDS)
@pytest.mark.parametrize("last", [8, 6], ids=["whole-chunks", "short-chunk"])
def test_mixed_histories(variant, last):
    """Uniform passes, adaptive passes, then a uniform pass on the film whose tiles differ -- with whole chunks, and with a
    short chunk, which closes the film: a later adaptive pass is refused and leaves the film untouched."""
    s = Setup(*variant)
    film, rep = s.film(), s.replay()
    for n in (4, 8):
        p, st = rep.uniform_pass(n), film.render(n)
        assert (st["rays"], st["paths"]) == (p["rays"], p["paths"])
        check_film(film, rep, f"{variant} uniform {n}")
    for k in range(3):
        adaptive_pass(film, rep, A.PASS, A.TAU, A.CAP, f"{variant} mixed, adaptive pass {k}")
    assert len(set(int(v) for v in rep.nt.ravel())) >= 2
    p, st = rep.uniform_pass(last), film.render(last)
    assert (st["rays"], st["paths"]) == (p["rays"], p["paths"])
    check_film(film, rep, f"{variant} uniform {last} on tiles that differ")
    if last % C == 0:
        adaptive_pass(film, rep, A.PASS, A.TAU, A.CAP, f"{variant} mixed, adaptive again")
        return
    assert film.status(A.TAU)["closed"] == 1
    before_img, before_st, before_nt = film.image(out_f64=True), film.status(A.TAU), film.tile_samples()
    with pytest.raises(_ffi.RayrsError) as e:
        film.render_adaptive(A.PASS, A.TAU, A.CAP)
    assert e.value.status == -1
    with pytest.raises(_ffi.RayrsError):
        film.render(4)
    assert same_bits(film.image(out_f64=True), before_img) and film.status(A.TAU) == before_st
    assert np.array_equal(film.tile_samples(), before_nt)


@pytest.mark.parametrize("variant", VARIANTS, ids=IDS)
def test_no_tile_active_and_what_is_refused(variant):
    s = Setup(*variant)
    film, rep = s.film(), s.replay()
    adaptive_pass(film, rep, A.PASS, A.TAU, A.CAP, f"{variant} first pass")
    # refused with nothing changed: n = 0, n that is no whole number of chunks, a negative or non-finite tau
    before_img, before_st = film.image(out_f64=True), film.status(A.TAU)
    for n, tau in ((0, 0.5), (6, 0.5), (8, -0.5), (8, float("nan")), (8, float("inf"))):
        with pytest.raises(_ffi.RayrsError) as e:
            film.render_adaptive(n, tau, A.CAP)
        assert e.value.status == -1, (n, tau)
    # a tau at which every pixel is converged (M = 2), and a cap that leaves no room: RAYRS_OK and nothing to do
    for tau, cap in ((1e6, A.CAP), (A.TAU, A.PASS), (A.TAU, A.PASS + 4)):
        assert rep.select(A.PASS, tau, cap) == []
        active, st = film.render_adaptive(A.PASS, tau, cap)
        assert active == 0 and all(v == 0 for v in st.values() if not isinstance(v, list)) and not any(st["surface_hits"]), (tau, cap, st)
    assert same_bits(film.image(out_f64=True), before_img) and film.status(A.TAU) == before_st
    check_film(film, rep, f"{variant} after the passes that did nothing")
    # an empty film below the cap: nothing selected, still empty
    empty = s.film()
    assert empty.render_adaptive(A.PASS, A.TAU, 4)[0] == 0 and not empty.tile_samples().any()
    with pytest.raises(_ffi.RayrsError):
        empty.image()


CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import _film, _film_adaptive as A, rayrs_amd
name, local_pool, state, out = sys.argv[3], int(sys.argv[4]), sys.argv[5], sys.argv[6]
cam_args, objs, heur, env = _film.DESCS[name](A.W, A.H)
scene = rayrs_amd.Scene(objs, 1e-6, 1e6, heur, env, device=0)
scene.set_tuning(local_pool=local_pool)
film = rayrs_amd.Film(scene, rayrs_amd.Camera(*cam_args), sample_chunk=A.C, max_bounces=A.BOUNCES, seed=A.SEED)
film.load(state)
active, st = film.render_adaptive(A.PASS, A.TAU, A.CAP)
np.save(out + ".npy", film.image(out_f64=True))
np.save(out + ".nt.npy", film.tile_samples())
json.dump(dict(active=active, rays=st["rays"], status=film.status(A.TAU)), open(out + ".json", "w"))
"""


@pytest.mark.parametrize("variant", VARIANTS, ids=IDS)
def test_a_checkpoint_of_a_film_whose_tiles_differ(variant, tmp_path):
    s = Setup(*variant)
    film, rep = s.film(), s.replay()
    for k in range(3):
        adaptive_pass(film, rep, A.PASS, A.TAU, A.CAP, f"{variant} pass {k}")
    assert len(set(int(v) for v in rep.nt.ravel())) >= 2
    path = tmp_path / "film.state"
    film.save(path)
    image = film.state()
    tiles_n = rep.ty * rep.tx
    assert os.path.getsize(path) == len(image) == 88 + tiles_n * 64 * 40 + tiles_n * 4
    saved_st = film.status(A.TAU)
    # a new Scene and Film in this process: the frame, the status and the N_t map, then one more pass
    s2 = Setup(*variant)
    again = s2.film()
    again.load(path)
    assert again.status(A.TAU) == saved_st
    check_film(again, rep, "loaded film")
    p, st = adaptive_pass(again, rep, A.PASS, A.TAU, A.CAP, f"{variant} continued in a new film")
    # a child process started fresh
    out = str(tmp_path / "child")
    r = subprocess.run([sys.executable, "-c", CHILD, os.path.dirname(HERE), HERE, variant[0], str(variant[1]), str(path), out],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    child = json.load(open(out + ".json"))
    assert (child["active"], child["rays"]) == (p["active_tiles"], p["rays"]) and child["status"] == again.status(A.TAU)
    assert same_bits(np.load(out + ".npy"), again.image(out_f64=True)) and np.array_equal(np.load(out + ".nt.npy"), rep.nt)
    # another version byte, truncated images, counts no sequence of passes leaves: refused, nothing changes
    before_img, before_st = again.image(out_f64=True), again.status(A.TAU)
    bad_version = bytearray(image)
    bad_version[4] ^= 3      # version 2 -> 1: the image version before the per-tile counts
    odd_count = bytearray(image)
    odd_count[-4] ^= 1       # the last tile's N_t is no whole number of chunks
    for bad in (bytes(bad_version), image[:-4], image[:-tiles_n * 4], image[:40], image + b"\0" * 4, bytes(odd_count)):
        with pytest.raises(_ffi.RayrsError) as e:
            again.set_state(bad)
        assert e.value.status == -1
    assert same_bits(again.image(out_f64=True), before_img) and again.status(A.TAU) == before_st
    check_film(again, rep, "after the refused images")


@pytest.mark.parametrize("variant", VARIANTS, ids=IDS)
def test_tile_shares_run_adaptively(variant):
    s = Setup(*variant)
    for r in range(3):
        film, rep = s.film(tile_rank=r, tile_ranks=3), s.replay(rank=r, ranks=3)
        for k in range(4):
            adaptive_pass(film, rep, A.PASS, A.TAU, A.CAP, f"{variant} share {r} pass {k}")
        mask = tiles.tile_mask(W, H, r, 3)
        assert np.array_equal(np.repeat(np.repeat(rep.share, 8, axis=0), 8, axis=1), mask)
        img, nt = film.image(out_f64=True), film.tile_samples()
        assert (img[~mask] == 0).all() and not np.signbit(img[~mask]).any()
        assert (nt[~rep.share] == 0).all() and (nt[rep.share] > 0).all()
        assert not (film.sample_map()[~mask]).any()


@pytest.mark.parametrize("variant", VARIANTS, ids=IDS)
def test_ragged_edges(variant):
    """61 x 19: the padding of the edge tiles is no pixel -- it never makes a tile active and counts nowhere."""
    s = Setup(*variant, w=61, h=19, samples=32)
    assert (s.cam.x_pixels(), s.cam.y_pixels()) == (61, 19)
    film, rep = s.film(), s.replay()
    seen = []
    for k in range(5):
        p, _ = adaptive_pass(film, rep, A.PASS, A.TAU, 32, f"{variant} 61x19 pass {k}")
        seen.append(p["active_tiles"])
    assert seen[0] == 8 * 3 and seen[-1] == 0, seen
    assert film.sample_map().shape == (19, 61)


def test_non_finite_pixels_keep_no_tile_active():
    """A scene of tests/_nonfinite.py whose frame has NaN pixels: a tile is inactive once each of its pixels is non-finite
    or converged, and stays so; the counts are the replay's."""
    desc = N.FAMILIES["emit_inf_red"][0]()
    cam_args, objs, heur, env = desc
    osc, ocam = _oracle.OracleScene(objs, 1e-6, 1e6, heur, env), _oracle.OracleCamera(*cam_args)
    rgb, it = A.traces(osc, ocam, 32, SEED, N.BUDGET)
    for local_pool in (0, 1):
        scene = rayrs_amd.Scene(objs, 1e-6, 1e6, heur, env, device=0)
        scene.set_tuning(local_pool=local_pool)
        film = rayrs_amd.Film(scene, rayrs_amd.Camera(*cam_args), sample_chunk=C, max_bounces=N.BUDGET, seed=SEED)
        rep = A.Replay(rgb, it, C)
        passes = []
        for k in range(5):
            p, _ = adaptive_pass(film, rep, A.PASS, A.TAU, 32, f"local_pool={local_pool} pass {k}", nan_aware=True)
            passes.append(p)
        assert passes[0]["nonfinite"] > 0 and passes[-1]["active_tiles"] == 0
        # tiles that held non-finite pixels and nothing unconverged were left out while others went on ...
        left_out = [(ty, tx) for q in passes[1:] if q["active_tiles"] for ty, tx in rep.tiles()
                    if not q["active"][ty, tx] and rep.tile_counts(ty, tx, A.TAU)[1] > 0 and rep.nt[ty, tx] < 32]
        assert left_out, "no tile with non-finite pixels was ever inactive below the cap"
        # ... and once inactive below the cap a tile never comes back
        for ty, tx in rep.tiles():
            act = [bool(q["active"][ty, tx]) for q in passes]
            assert act == sorted(act, reverse=True), (ty, tx, act)
        st = film.status(A.TAU)
        assert st["nan_pixels"] > 0 and st["nonfinite"] >= st["nan_pixels"]


def test_the_fast_walk_takes_adaptive_passes():
    desc = _film.mesh_desc(32, 24)
    cam_args, objs, heur, env = desc
    scene = rayrs_amd.Scene(objs, 1e-6, 1e6, heur, env, device=0)
    cam = rayrs_amd.Camera(*cam_args)
    osc, ocam = _film.oracle_of(desc)
    rgb, it = A.traces(osc.use_product_walk(scene, fast=True), ocam, 32, traversal=2)
    film = rayrs_amd.Film(scene, cam, sample_chunk=C, max_bounces=BOUNCES, seed=SEED, fast_traversal=True)
    rep = A.Replay(rgb, it, C)
    seen = []
    for k in range(5):
        p, st = adaptive_pass(film, rep, A.PASS, A.TAU, 32, f"fast walk pass {k}")
        assert p["active_tiles"] == 0 or st["exact_walk"] == 0
        seen.append(p["active_tiles"])
    assert seen[0] == 12 and seen[-1] == 0


@pytest.mark.parametrize("variant", VARIANTS, ids=IDS)
def test_a_plain_render_between_two_adaptive_passes(variant):
    """It shares the pool, the item sums and the counters with the film."""
    s = Setup(*variant)
    film, rep = s.film(), s.replay()
    for k in range(2):
        adaptive_pass(film, rep, A.PASS, A.TAU, A.CAP, f"{variant} pass {k}")
    ref, ost = s.osc.render(s.ocam, 5, BOUNCES, SEED)
    img, st = rayrs_amd.render(s.scene, s.cam, 5, BOUNCES, SEED, out_f64=True)
    assert same_bits(img, ref) and st["rays"] == ost["rays"]
    adaptive_pass(film, rep, A.PASS, A.TAU, A.CAP, f"{variant} pass behind the plain render")
    img, st = rayrs_amd.render(s.scene, s.cam, 5, BOUNCES, SEED, out_f64=True)
    assert same_bits(img, ref) and st["rays"] == ost["rays"]


def run_cli(args, cwd):
    cwd.mkdir()
    r = subprocess.run([CLI] + args, cwd=cwd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout, (cwd / "diffuse_single_sphere.png").read_bytes(), (cwd / "diffuse_single_sphere.hdr").read_bytes()


def test_command_line_adaptive(tmp_path):
    io.save_hdr(tmp_path / "env.hdr", procedural.make_hdri(64, 32))
    base = [str(tmp_path / "env.hdr"), "64", "--scene", "diffuse_single_sphere", "--seed", "9", "--pass", "8", "--until-noise", "0.5"]
    cam_args, objs, heur = scenes.diffuse_single_sphere()
    scene = rayrs_amd.Scene(objs, 1e-6, 1e6, heur, io.load_hdr(tmp_path / "env.hdr"), device=0)
    cam = rayrs_amd.Camera(*cam_args)

    def files_of(film, name):
        img = film.image()
        io.save_png(tmp_path / f"{name}.png", io.to_raw_bytes(img)[0])
        io.save_hdr(tmp_path / f"{name}.hdr", img)
        return (tmp_path / f"{name}.png").read_bytes(), (tmp_path / f"{name}.hdr").read_bytes()

    # with --adaptive: the per-tile counts render_until(adaptive=True) stops at, and the files of that film
    film = rayrs_amd.Film(scene, cam, sample_chunk=4, max_bounces=50, seed=9)
    seen = []
    st, why = rayrs_amd.render_until(film, 0.5, 0.0, pass_samples=8, max_samples=64, adaptive=True,
                                     on_pass=lambda f, x: seen.append(x["active_tiles"]))
    per_pixel = film.sample_map()
    assert len(np.unique(per_pixel)) >= 2, "the program's frame does not exercise the rule at this tau"
    out, png, hdr = run_cli(base + ["--adaptive"], tmp_path / "adaptive")
    assert [int(v) for v in re.findall(r"Pass: (\d+) active tiles", out)] == seen
    m = re.search(r"Samples per pixel: min (\d+), mean ([0-9.]+), max (\d+)", out)
    assert m and (int(m.group(1)), int(m.group(3))) == (int(per_pixel.min()), int(per_pixel.max())) == (st["tile_samples_min"], st["tile_samples_max"])
    assert abs(float(m.group(2)) - per_pixel.mean()) < 1e-3 and st["pixel_samples"] == int(per_pixel.sum())
    assert (png, hdr) == files_of(film, "adaptive_lib")
    # --adaptive may stand anywhere among the options
    out2, png2, hdr2 = run_cli(base[:2] + ["--adaptive"] + base[2:], tmp_path / "adaptive_first")
    assert (png2, hdr2) == (png, hdr)
    # without the flag: the uniform film's passes, output and files
    film = rayrs_amd.Film(scene, cam, sample_chunk=4, max_bounces=50, seed=9)
    st, why = rayrs_amd.render_until(film, 0.5, 0.0, pass_samples=8, max_samples=64)
    out, png_u, hdr_u = run_cli(base, tmp_path / "uniform")
    assert int(re.search(r"Samples per pixel: (\d+)\n", out).group(1)) == st["samples"] and "active tiles" not in out
    assert (png_u, hdr_u) == files_of(film, "uniform_lib")
    # --adaptive needs a tau
    r = subprocess.run([CLI] + base[:8] + ["--adaptive"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 1 and "--until-noise" in r.stderr
