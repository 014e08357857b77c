"""The direct-lit films (include/rayrs_hip.h DIRECT-LIT FILMS) on the GPU, bit for bit and count for count.

At 20 x 12 in chunks of 2 -- 3 x 2 tiles, four padded columns and four padded rows -- the expectation is the plain-Python readings'
per-sample values (tests/_film_direct.py), folded by _film.expectation, _film.noise_counts and _film_adaptive.Replay: nothing in it
calls the library.  The families are tests/test_gpu_sky.py's `room` under the studio map with its two lamps (local-pool-sized: the
default walk whatever is asked) and `mesh1_light` under the gradient map with its lamp (streams, hot group, a fast walk of its
own), each as a _direct film (the list) and as a _sky film (the list and SKY), the mesh scene on both walks.

At 472 x 456 in chunks of 4 on `mesh1_light` -- 3363 tiles, at 20 samples 1,076,160 items, the smallest film whose pass needs two
launches and an accumulate per tile range -- there is no Python reading: the reference is render_lit(direct=True), which
tests/test_gpu_direct.py and tests/test_gpu_sky.py hold to the readings."""
import functools
import os
import subprocess

import numpy as np
import pytest

import _film
import _film_adaptive
import _film_direct as FD
import _guided as G
import rayrs_amd
from rayrs_amd import SKY, _ffi, io, procedural, scenes
from test_gpu_sky import family

pytestmark = pytest.mark.gpu

CLI = os.path.join(os.path.dirname(os.path.abspath(rayrs_amd.__file__)), "rayrs")
SKY_OF = {"room": "studio", "mesh1_light": "gradient"}
CASES = [(name, kernel, fast) for name, fasts in (("room", (False,)), ("mesh1_light", (False, True))) for kernel in FD.KERNELS for fast in fasts]
PIXELS = FD.W * FD.H
INVALID_ARG, UNSUPPORTED = -1, -5


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64 if np.asarray(x).dtype == np.float64 else np.uint32)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def scene_of(name):
    f = family(name, SKY_OF[name])
    FD.register_fast_walk(name, f.readings[True].osc)
    assert tuple(f.lists["two" if name == "room" else "lamp"]) == FD.description(name)[4]
    return f.scene


def camera_of(name):
    return rayrs_amd.Camera(*FD.description(name)[0])


def make_film(name, kernel, fast=False, **kw):
    return rayrs_amd.Film(scene_of(name), camera_of(name), sample_chunk=FD.C, seed=FD.SEED, fast_traversal=fast, lights=FD.lights(name, kernel),
                          direct=True, **kw)


def reading(name, kernel, fast):
    """The reading of the walk the film takes: the room is local-pool-sized and takes the default walk whatever is asked."""
    scene_of(name)
    return FD.paths(name, kernel, fast and name != "room")


def check_status(film, s1, s2, m, n, rays, closed, what):
    for tau in _film.TAUS:
        st = film.status(tau)
        unc, nonf = _film.noise_counts(s1, s2, m, tau)
        assert (st["unconverged"], st["nonfinite"]) == (unc, nonf), (what, tau, st)
        assert (st["samples"], st["full_chunks"], st["closed"]) == (n, n // FD.C, int(closed)), (what, st)
        assert st["rays"] == rays and st["paths"] == PIXELS * n, (what, st, rays)


# ---- 1. passes and status

@pytest.mark.parametrize("name,kernel,fast", CASES)
def test_passes_and_status_are_the_readings(name, kernel, fast):
    rgb, q = reading(name, kernel, fast)
    film = make_film(name, kernel, fast)
    assert film.lights == FD.lights(name, kernel)
    n = 0
    for step in (2, 4, 3):
        st = film.render(step)
        n += step
        frame, s1, s2, m = _film.expectation(rgb, FD.C, n)
        assert np.isfinite(frame).all()
        assert same(film.image(out_f64=True), frame), (name, kernel, fast, n)
        assert same(film.image(), frame.astype(np.float32)), (name, kernel, fast, n)
        assert st["rays"] == int(q[:, :, n - step:n].sum()) and st["paths"] == PIXELS * step, (n, st)
        assert st["exact_walk"] == int(not (fast and name != "room")), st
        for zero in ("kernel_launches", "interior_visits", "tri_tests", "local_pool", "hot_group", "direct_rays", "escaped_paths"):
            assert st[zero] == 0, (zero, st)
        check_status(film, s1, s2, m, n, int(q[:, :, :n].sum()), step % FD.C != 0, (name, kernel, fast, n))
    with pytest.raises(_ffi.RayrsError) as e:   # the pass of 3 closed the film
        film.render(2)
    assert e.value.status == INVALID_ARG
    assert same(film.image(out_f64=True), _film.expectation(rgb, FD.C, 9)[0])


def test_a_pass_longer_than_one_launch_per_tile_is_refused_and_leaves_the_film():
    film = make_film("room", "sky")
    film.render(2)
    before = film.state()
    for call in (lambda: film.render(2 * 16385), lambda: film.render_adaptive(2 * 16385, 0.1)):
        with pytest.raises(_ffi.RayrsError) as e:
            call()
        assert e.value.status == UNSUPPORTED
    assert film.state() == before


# ---- 2. partitions and checkpoint

@pytest.mark.parametrize("name,kernel", [("room", "sky"), ("mesh1_light", "direct")])
def test_partitions_and_a_checkpoint_leave_the_same_image(name, kernel, tmp_path):
    states = []
    for parts in ((6,), (2, 4), (4, 2), (2, 2, 2)):
        film = make_film(name, kernel)
        for n in parts:
            film.render(n)
        states.append(film.state())
    assert len(states[0]) == 88 + 6 * 5 * 64 * 8 + 6 * 4
    assert all(s == states[0] for s in states[1:])
    first = make_film(name, kernel)
    first.render(2)
    first.save(tmp_path / "film.state")
    second = make_film(name, kernel)
    second.load(tmp_path / "film.state")
    second.render(4)
    assert second.state() == states[0]
    rgb, q = reading(name, kernel, False)
    assert same(second.image(out_f64=True), _film.expectation(rgb, FD.C, 6)[0]) and second.status(0.2)["rays"] == int(q[:, :, :6].sum())


# ---- 3. adaptive passes

SEQUENCE = ("adaptive", "uniform", "adaptive", "adaptive", "adaptive")   # passes of 2 under a cap of 8, a uniform pass in between
TAU_GRID = tuple(float(t) for t in np.round(np.geomspace(0.02, 0.9, 24), 3)) + (0.95, 0.98, 0.99, 0.999, 0.999999)


def replay_sequence(rgb, q, tau):
    """The replay's passes of SEQUENCE at tau: [(kind, what the replay expects after it)]."""
    rep, out = _film_adaptive.Replay(rgb, q, c=FD.C), []
    for kind in SEQUENCE:
        if kind == "adaptive":
            out.append((kind, rep.adaptive_pass(2, tau, 8)))
        elif int(rep.nt.max()) + 2 <= 8:
            out.append((kind, rep.uniform_pass(2, tau)))
    return out


@functools.lru_cache(maxsize=None)
def adaptive_tau(name, kernel, fast):
    """(tau, splits): a tau of TAU_GRID, chosen from the reading alone, at which some adaptive pass of SEQUENCE selects some but not
    all of the six tiles; splits is False where the reading has none.  (A tau of 1 or more selects nothing once a tile has two
    chunks: with non-negative chunk sums the predicate then always holds.)"""
    rgb, q = reading(name, kernel, fast)
    for tau in TAU_GRID:
        if any(kind == "adaptive" and 0 < want["active_tiles"] < 6 for kind, want in replay_sequence(rgb, q, tau)):
            return tau, True
    return 0.5, False


@pytest.mark.parametrize("name,kernel,fast", CASES)
def test_adaptive_passes_are_the_replay(name, kernel, fast):
    """The room's readings split the six tiles, and the test asserts that they do.  mesh1_light's do not, at any tau: at 20 x 12
    every tile of that frame holds a pixel one of whose chunk sums is +0 beside a positive one, which is unconverged at every
    tau below 1 with two, three and four chunks alike -- so under a cap of 8 its adaptive passes take all six tiles or none, and
    what these cases hold is the replay's counts, frames and status with lists of all six tiles.  Partial lists on mesh1_light
    are the large frame's (test_large_adaptive_passes_leave_every_tile_at_its_own_count)."""
    rgb, q = reading(name, kernel, fast)
    tau, splits = adaptive_tau(name, kernel, fast)
    assert splits == (name == "room"), (name, kernel, fast, tau)
    film = make_film(name, kernel, fast)
    rays = paths = 0
    partial = False
    for kind, want in replay_sequence(rgb, q, tau):
        if kind == "adaptive":
            active, st = film.render_adaptive(2, tau, 8)
            assert active == want["active_tiles"], (kind, active, want["active_tiles"])
            partial = partial or 0 < active < 6
        else:
            st = film.render(2)
        rays, paths = rays + want["rays"], paths + want["paths"]
        assert st["rays"] == want["rays"] and st["paths"] == want["paths"], (kind, st, want["rays"], want["paths"])
        assert np.array_equal(film.tile_samples(), want["nt"]), kind
        assert same(film.image(out_f64=True), want["frame"]), kind
        got = film.status(tau)
        assert (got["unconverged"], got["nonfinite"], got["rays"], got["paths"]) == (want["unconverged"], want["nonfinite"], rays, paths), (kind, got)
        assert got["samples"] == int(want["nt"].max())
    assert partial == splits


# ---- 4. tile shares

@pytest.mark.parametrize("name,kernel", [("room", "direct"), ("mesh1_light", "sky")])
def test_tile_shares_hold_their_tiles_of_the_whole_frame(name, kernel):
    rgb, q = reading(name, kernel, False)
    frame = _film.expectation(rgb, FD.C, 6)[0]
    total = 0
    for rank in (0, 1):
        film = make_film(name, kernel, tile_rank=rank, tile_ranks=2)
        film.render(2), film.render(4)
        rep = _film_adaptive.Replay(rgb, q, c=FD.C, rank=rank, ranks=2)
        mine = rep.per_pixel(rep.share)
        want = np.where(mine[..., None], frame, 0.0)
        assert same(film.image(out_f64=True), want), rank
        st = film.status(0.2)
        assert st["rays"] == int(q[:, :, :6][mine].sum()) and st["paths"] == int(mine.sum()) * 6
        total += st["rays"]
    assert total == int(q[:, :, :6].sum())


# ---- 5. the empty list, 6. not vacuous

@pytest.mark.parametrize("name", ["room", "mesh1_light"])
def test_an_empty_list_is_a_plain_film_and_a_list_is_not(name):
    scene, cam = scene_of(name), camera_of(name)
    plain = rayrs_amd.Film(scene, cam, sample_chunk=FD.C, seed=FD.SEED)
    empty = rayrs_amd.Film(scene, cam, sample_chunk=FD.C, seed=FD.SEED, lights=[], direct=True)
    for film in (plain, empty):
        film.render(2), film.render(4)
    assert empty.state()[88:] == plain.state()[88:]   # the records and the tile counts (the header holds `rays`: direct's has shadow rays)
    assert np.array_equal(empty.tile_samples(), plain.tile_samples())
    img, _ = rayrs_amd.render(scene, cam, spp=6, seed=FD.SEED, sample_chunk=FD.C, out_f64=True)
    assert same(empty.image(out_f64=True), img) and same(plain.image(out_f64=True), img)
    for kernel in FD.KERNELS:
        lit = make_film(name, kernel)
        lit.render(2), lit.render(4)
        got = lit.image(out_f64=True)
        assert np.isfinite(got).all() and (bits(got) != bits(img)).any(axis=2).sum() >= 10, kernel


# ---- 7. downstream

@pytest.mark.parametrize("name,kernel", [("room", "sky"), ("mesh1_light", "direct")])
def test_noise_filter_and_history_read_the_records(name, kernel):
    rgb, q = reading(name, kernel, False)
    frame, s1, s2, m = _film.expectation(rgb, FD.C, 6)
    film = make_film(name, kernel)
    film.render(2), film.render(4)
    plane = G.noise_plane(s1, s2, np.full((2, 3), 6), FD.C)
    assert same(film.noise(), plane)
    color, noise, feats = film.image(out_f64=True), film.noise(), film.features()
    sigmas = dict(sigma_normal=0.5, sigma_albedo=0.2, sigma_depth=2.0, sigma_luminance=4.0)
    want = rayrs_amd.denoise_guided(color, noise, feats["normal"], feats["albedo"], feats["depth"], levels=2, **sigmas)
    got = film.denoised_guided(levels=2, out_f64=True, **sigmas)
    assert same(got, want) and not same(got, color)
    cam = camera_of(name)
    a, b = rayrs_amd.History(), rayrs_amd.History()
    a.push(film)
    b.push_image(cam, color, noise, np.full((FD.H, FD.W), 6.0), feats["normal"], feats["albedo"], feats["depth"], feats["coverage"], feats["object"])
    for x, y in zip(a.read(), b.read()):
        assert same(x, y)
    assert same(film.image(out_f64=True), frame)


# ---- 8. neighbours unharmed

def test_the_neighbours_on_the_shared_scratch_keep_their_bits():
    name = "mesh1_light"
    f = family(name, SKY_OF[name])
    scene, cam = scene_of(name), camera_of(name)
    lamps = FD.lights(name, "direct")

    def neighbours():
        plain = rayrs_amd.Film(scene, cam, sample_chunk=FD.C, seed=FD.SEED)
        plain.render(4)
        return (plain.state(), rayrs_amd.render(scene, cam, spp=4, seed=FD.SEED, out_f64=True)[0],
                rayrs_amd.render_lit(scene, cam, 4, lamps, seed=FD.SEED, sample_chunk=2, direct=True),
                f.scene.radiance(f.o, f.d, samples=3, seed=FD.SEED, lights=lamps + [SKY], direct=True))
    before = neighbours()
    for kernel in FD.KERNELS:
        film = make_film(name, kernel)
        film.render(2), film.render_adaptive(2, 0.1, 8), film.render(2)
    after = neighbours()
    assert before[0] == after[0]
    for x, y in zip(before[1:], after[1:]):
        assert same(x, y)


# ---- the large frame: two launches a pass, an accumulate per tile range

BIG_W, BIG_H, BIG_C = 472, 456, 4


@functools.lru_cache(maxsize=None)
def big_camera():
    cam_args = scenes.mesh_scene(1, rayrs_amd.api.Material.LambertianDiffuse((0.8, 0.8, 0.8)), area_light=True)[0]
    return rayrs_amd.Camera(*scenes.camera_for_resolution(cam_args, BIG_W, BIG_H))


@functools.lru_cache(maxsize=None)
def big_reference(kernel, samples):
    img, cnt = rayrs_amd.render_lit(scene_of("mesh1_light"), big_camera(), samples, FD.lights("mesh1_light", kernel), seed=FD.SEED, sample_chunk=BIG_C,
                                    queries=True, direct=True)
    img.setflags(write=False), cnt.setflags(write=False)
    return img, cnt


def big_film(kernel):
    return rayrs_amd.Film(scene_of("mesh1_light"), big_camera(), sample_chunk=BIG_C, seed=FD.SEED, lights=FD.lights("mesh1_light", kernel), direct=True)


@pytest.mark.parametrize("kernel", FD.KERNELS)
def test_a_pass_of_two_launches_is_the_image_forms_frame(kernel):
    assert ((BIG_W + 7) // 8) * ((BIG_H + 7) // 8) * 64 * 5 > 1 << 20
    img, cnt = big_reference(kernel, 20)
    for parts in ((20,), (8, 12)):
        film = big_film(kernel)
        for n in parts:
            film.render(n)
        assert same(film.image(out_f64=True), img), (kernel, parts)
        st = film.status(0.2)
        assert st["rays"] == int(cnt.sum(dtype=np.uint64)) and st["paths"] == BIG_W * BIG_H * 20, (kernel, parts, st)


@pytest.mark.parametrize("kernel", FD.KERNELS)
def test_large_adaptive_passes_leave_every_tile_at_its_own_count(kernel):
    film = big_film(kernel)
    film.render(8)
    n_tiles = ((BIG_W + 7) // 8) * ((BIG_H + 7) // 8)
    # a tau at which film.status reports some but not all pixels unconverged: the one of the list that leaves the fewest
    counts = {t: film.status(t)["unconverged"] for t in (0.1, 0.2, 0.3, 0.5, 0.7, 0.8, 0.9, 0.95)}
    some = {t: u for t, u in counts.items() if 0 < u < BIG_W * BIG_H}
    assert some, counts
    tau = min(some, key=some.get)
    active, _ = film.render_adaptive(4, tau, 12)
    assert 0 < active < n_tiles, (tau, active, counts)
    film.render_adaptive(4, tau, 12)   # (the cap: no tile is taken twice)
    nt = film.tile_samples()
    assert sorted(np.unique(nt)) == [8, 12]
    per_pixel = np.repeat(np.repeat(nt, 8, axis=0), 8, axis=1)[:BIG_H, :BIG_W]
    got = film.image(out_f64=True)
    rays = 0
    for n in (8, 12):
        img, cnt = big_reference(kernel, n)
        px = per_pixel == n
        assert np.array_equal(bits(got)[px], bits(img)[px]), (kernel, n)
        rays += int(cnt[px].sum(dtype=np.uint64))
    assert film.status(tau)["rays"] == rays


# ---- 11. the command line

def test_the_command_line_makes_a_sky_lit_film_and_keeps_its_ordinary_files(tmp_path):
    io.save_hdr(tmp_path / "env.hdr", procedural.make_hdri(128, 64))
    name = "diffuse_single_sphere"
    common = [CLI, str(tmp_path / "env.hdr"), "6", "--seed", "77", "--scene", name]
    for opt in ("--sky", "--direct"):
        bad = tmp_path / ("bad" + opt)
        bad.mkdir()
        r = subprocess.run(common + [opt], cwd=bad, capture_output=True, text=True, timeout=600)
        assert r.returncode == 2 and opt in r.stderr and os.listdir(bad) == [], (opt, r.stderr)
    bad = tmp_path / "no_lamp"
    bad.mkdir()
    r = subprocess.run(common + ["--pass", "2", "--direct"], cwd=bad, capture_output=True, text=True, timeout=600)
    assert r.returncode == 2 and "--direct" in r.stderr and os.listdir(bad) == [], r.stderr
    dirs = {}
    for sub, args in (("plain", []), ("sky", ["--sky"]), ("both", ["--direct", "--sky"])):
        dirs[sub] = tmp_path / sub
        dirs[sub].mkdir()
        r = subprocess.run(common + ["--pass", "2", "--sample-chunk", "2"] + args, cwd=dirs[sub], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        assert sorted(os.listdir(dirs[sub])) == [name + ".hdr", name + ".png"]
    cam_args, objs, heur = scenes.diffuse_single_sphere()
    scene, cam = rayrs_amd.Scene(objs, 1e-6, 1e6, heur, io.load_hdr(tmp_path / "env.hdr"), device=0), rayrs_amd.Camera(*cam_args)
    for sub, kw in (("plain", {}), ("sky", dict(lights=[SKY], direct=True)), ("both", dict(lights=[SKY], direct=True))):
        film = rayrs_amd.Film(scene, cam, sample_chunk=2, seed=77, **kw)
        for _ in range(3):
            film.render(2)
        io.save_hdr(tmp_path / "want.hdr", film.image())
        assert (dirs[sub] / (name + ".hdr")).read_bytes() == (tmp_path / "want.hdr").read_bytes(), sub
    assert (dirs["plain"] / (name + ".hdr")).read_bytes() != (dirs["sky"] / (name + ".hdr")).read_bytes()
