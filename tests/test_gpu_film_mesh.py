"""The mesh-lit films (include/rayrs_hip.h MESH-LIT FILMS AND BAKES) on the GPU, bit for bit and count for count.

At 20 x 12 in chunks of 2 -- 3 x 2 tiles, four padded columns and four padded rows -- the expectation is the plain-Python reading's
per-sample values (tests/_film_mesh.py over tests/_mesh.py), folded by _film.expectation, _film.noise_counts and
_film_adaptive.Replay: nothing in it calls the library, and every expected value is finite, so each comparison is of bits.  The
families are tests/test_gpu_mesh_lights.py's `room`, `small` (local-pool-sized: asked for the fast walk, it takes the default one)
and `mesh1` (on both walks), each without and with the sky.

At 472 x 456 in chunks of 4 on `mesh1` -- 3363 tiles, at 20 samples 1,076,160 items, the smallest film whose pass needs two launches
-- and at 96 x 64, where mesh1's adaptive lists are partial, there is no Python reading: the reference is
render_lit(direct=True, mesh=group), which tests/test_gpu_mesh_lights.py holds to the reading."""
import functools

import numpy as np
import pytest

import _film
import _film_adaptive
import _film_mesh as FM
import _guided as G
import rayrs_amd
from rayrs_amd import SKY, _ffi, scenes
from test_gpu_mesh_lights import family, mesh1_objects

pytestmark = pytest.mark.gpu

# (family, sky, the walk asked for): small is local-pool-sized and takes the default walk whatever is asked
CASES = [(name, sky, fast) for name, fasts in (("room", (False,)), ("small", (True,)), ("mesh1", (False, True))) for sky in (False, True)
         for fast in fasts]
PIXELS = FM.W * FM.H
INVALID_ARG, UNSUPPORTED = -1, -5


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64 if np.asarray(x).dtype == np.float64 else np.uint32)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def fam(name):
    f = family(name)
    FM.register_fast_walk(name, f.readings[True])
    assert tuple(f.tris) == FM.description(name)[3] and tuple(f.lists[FM.LIST_OF[name]]) == FM.description(name)[4]
    return f


def camera_of(name):
    return rayrs_amd.Camera(*FM.description(name)[0])


def walk_taken(name, fast):
    return bool(fast and name == "mesh1")


def make_film(name, sky, fast=False, mesh="group", **kw):
    f = fam(name)
    return rayrs_amd.Film(f.scene, camera_of(name), sample_chunk=FM.C, seed=FM.SEED, fast_traversal=fast, lights=FM.lights(name, sky), direct=True,
                          mesh=f.mesh if mesh == "group" else mesh, **kw)


def reading(name, sky, fast):
    fam(name)
    rgb, q = FM.image_paths(name, sky, walk_taken(name, fast))
    assert rgb.shape == (FM.H, FM.W, FM.N_MAX, 3) and np.isfinite(rgb).all()
    return rgb, q


def check_status(film, s1, s2, m, n, rays, closed, what):
    for tau in _film.TAUS:
        st = film.status(tau)
        unc, nonf = _film.noise_counts(s1, s2, m, tau)
        assert (st["unconverged"], st["nonfinite"]) == (unc, nonf), (what, tau, st)
        assert (st["samples"], st["full_chunks"], st["closed"]) == (n, n // FM.C, int(closed)), (what, st)
        assert st["rays"] == rays and st["paths"] == PIXELS * n, (what, st, rays)


# ---- 1. passes and status

@pytest.mark.parametrize("name,sky,fast", CASES)
def test_passes_and_status_are_the_readings(name, sky, fast):
    rgb, q = reading(name, sky, fast)
    film = make_film(name, sky, fast)
    assert film.lights == FM.lights(name, sky) and film.mesh is fam(name).mesh
    n = 0
    for step in (2, 4, 3):
        st = film.render(step)
        n += step
        frame, s1, s2, m = _film.expectation(rgb, FM.C, n)
        assert np.isfinite(frame).all()
        assert same(film.image(out_f64=True), frame), (name, sky, fast, n)
        assert same(film.image(), frame.astype(np.float32)), (name, sky, fast, n)
        assert st["rays"] == int(q[:, :, n - step:n].sum()) and st["paths"] == PIXELS * step, (n, st)
        assert st["exact_walk"] == int(not walk_taken(name, fast)), st
        check_status(film, s1, s2, m, n, int(q[:, :, :n].sum()), step % FM.C != 0, (name, sky, fast, n))
    with pytest.raises(_ffi.RayrsError) as e:   # the pass of 3 closed the film
        film.render(2)
    assert e.value.status == INVALID_ARG
    assert same(film.image(out_f64=True), _film.expectation(rgb, FM.C, 9)[0])


# ---- 2. partitions and checkpoint

@pytest.mark.parametrize("name,sky", [("room", True), ("small", False), ("mesh1", False), ("mesh1", True)])
def test_partitions_and_a_checkpoint_leave_the_same_image(name, sky, tmp_path):
    states = []
    for parts in ((6,), (2, 4), (4, 2), (2, 2, 2)):
        film = make_film(name, sky)
        for n in parts:
            film.render(n)
        states.append(film.state())
    assert len(states[0]) == 88 + 6 * 5 * 64 * 8 + 6 * 4
    assert all(s == states[0] for s in states[1:])
    first = make_film(name, sky)
    first.render(2)
    first.save(tmp_path / "film.state")
    second = make_film(name, sky)
    second.load(tmp_path / "film.state")
    second.render(4)
    assert second.state() == states[0]
    rgb, q = reading(name, sky, False)
    assert same(second.image(out_f64=True), _film.expectation(rgb, FM.C, 6)[0]) and second.status(0.2)["rays"] == int(q[:, :, :6].sum())


# ---- 3. adaptive passes

SEQUENCE = ("adaptive", "uniform", "adaptive", "adaptive", "adaptive")   # passes of 2 under a cap of 8, a uniform pass in between
TAU_GRID = tuple(float(t) for t in np.round(np.geomspace(0.02, 0.9, 24), 3)) + (0.95, 0.98, 0.99, 0.999, 0.999999)


def replay_sequence(rgb, q, tau):
    """The replay's passes of SEQUENCE at tau: [(kind, what the replay expects after it)]."""
    rep, out = _film_adaptive.Replay(rgb, q, c=FM.C), []
    for kind in SEQUENCE:
        if kind == "adaptive":
            out.append((kind, rep.adaptive_pass(2, tau, 8)))
        elif int(rep.nt.max()) + 2 <= 8:
            out.append((kind, rep.uniform_pass(2, tau)))
    return out


@functools.lru_cache(maxsize=None)
def adaptive_tau(name, sky, fast):
    """(tau, splits): the first tau of TAU_GRID, chosen from the reading alone, at which some adaptive pass of SEQUENCE selects some
    but not all of the six tiles; splits is False where the reading has none."""
    rgb, q = reading(name, sky, fast)
    for tau in TAU_GRID:
        if any(kind == "adaptive" and 0 < want["active_tiles"] < 6 for kind, want in replay_sequence(rgb, q, tau)):
            return tau, True
    return 0.5, False


@pytest.mark.parametrize("name,sky,fast", CASES)
def test_adaptive_passes_are_the_replay(name, sky, fast):
    """room's and small's readings split the six tiles (at tau 0.763 to 0.9 the third adaptive pass takes five), and the test
    asserts that they do.  mesh1's do not, at any tau of the grid and under any cap the nine samples of the reading allow: as on
    tests/test_gpu_film_direct.py's mesh1_light, every tile of this frame holds a pixel one of whose chunk sums is +0 beside a
    positive one, which is unconverged at every tau below 1 with two, three and four chunks alike, and at a tau of 1 or more nothing
    is once a tile has two chunks -- so its adaptive passes take all six tiles or none, which the test asserts too, and what these
    cases hold is the replay's counts, frames and status with lists of all six tiles.  Partial lists on mesh1, on both walks, are
    test_mesh1s_partial_lists_leave_every_tile_at_its_own_count's."""
    rgb, q = reading(name, sky, fast)
    tau, splits = adaptive_tau(name, sky, fast)
    assert splits == (name != "mesh1"), (name, sky, fast, tau)
    film = make_film(name, sky, fast)
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
        assert np.isfinite(want["frame"]).all()
        assert same(film.image(out_f64=True), want["frame"]), kind   # (tile by tile at its own count: the replay's frame)
        got = film.status(tau)
        assert (got["unconverged"], got["nonfinite"], got["rays"], got["paths"]) == (want["unconverged"], want["nonfinite"], rays, paths), (kind, got)
        assert got["samples"] == int(want["nt"].max())
    assert partial == splits


MID_W, MID_H, MID_C = 96, 64, 4


@pytest.mark.parametrize("sky,fast", [(False, False), (True, True)])
def test_mesh1s_partial_lists_leave_every_tile_at_its_own_count(sky, fast):
    """96 x 64 in chunks of 4, 96 tiles: a pass of 8, then adaptive passes of 4 under a cap of 12 at a tau at which film.status
    reports some but not all pixels unconverged.  Every tile then holds 8 or 12 samples and reads render_lit(mesh=)'s pixels at
    its own count."""
    f = fam("mesh1")
    cam = rayrs_amd.Camera(*scenes.camera_for_resolution(mesh1_objects()[0], MID_W, MID_H))
    lights = FM.lights("mesh1", sky)
    film = rayrs_amd.Film(f.scene, cam, sample_chunk=MID_C, seed=FM.SEED, fast_traversal=fast, lights=lights, direct=True, mesh=f.mesh)
    film.render(8)
    n_tiles = (MID_W // 8) * (MID_H // 8)
    counts = {t: film.status(t)["unconverged"] for t in (0.1, 0.2, 0.3, 0.5, 0.7, 0.8, 0.9, 0.95)}
    some = {t: u for t, u in counts.items() if 0 < u < MID_W * MID_H}
    assert some, counts
    tau = min(some, key=some.get)
    active, _ = film.render_adaptive(4, tau, 12)
    assert 0 < active < n_tiles, (tau, active, counts)
    film.render_adaptive(4, tau, 12)   # (the cap: no tile is taken twice)
    nt = film.tile_samples()
    assert sorted(np.unique(nt)) == [8, 12]
    per_pixel = np.repeat(np.repeat(nt, 8, axis=0), 8, axis=1)[:MID_H, :MID_W]
    got = film.image(out_f64=True)
    rays = 0
    for n in (8, 12):
        img, cnt = rayrs_amd.render_lit(f.scene, cam, n, lights, seed=FM.SEED, sample_chunk=MID_C, fast_traversal=fast, queries=True, direct=True,
                                        mesh=f.mesh)
        px = per_pixel == n
        assert np.isfinite(img).all() and np.array_equal(bits(got)[px], bits(img)[px]), (sky, fast, n)
        rays += int(cnt[px].sum(dtype=np.uint64))
    assert film.status(tau)["rays"] == rays


# ---- 4. tile shares

@pytest.mark.parametrize("name,sky,ranks", [("room", False, 2), ("mesh1", True, 3), ("small", True, 3), ("mesh1", False, 2)])
def test_tile_shares_hold_their_tiles_of_the_whole_frame(name, sky, ranks):
    rgb, q = reading(name, sky, False)
    frame = _film.expectation(rgb, FM.C, 6)[0]
    total = 0
    for rank in range(ranks):
        film = make_film(name, sky, tile_rank=rank, tile_ranks=ranks)
        film.render(2), film.render(4)
        rep = _film_adaptive.Replay(rgb, q, c=FM.C, rank=rank, ranks=ranks)
        mine = rep.per_pixel(rep.share)
        want = np.where(mine[..., None], frame, 0.0)
        assert same(film.image(out_f64=True), want), rank   # (the rest read +0)
        st = film.status(0.2)
        assert st["rays"] == int(q[:, :, :6][mine].sum()) and st["paths"] == int(mine.sum()) * 6
        total += st["rays"]
    assert total == int(q[:, :, :6].sum())


# ---- 5. the empty group

@pytest.mark.parametrize("name", ["room", "mesh1"])
def test_an_empty_group_is_the_direct_or_the_sky_film_and_a_group_is_not(name):
    f = fam(name)
    cam = camera_of(name)
    empty = f.scene.mesh_lights([])
    for sky in (False, True):
        lights = FM.lights(name, sky)
        plain = rayrs_amd.Film(f.scene, cam, sample_chunk=FM.C, seed=FM.SEED, lights=lights, direct=True)
        assert plain.mesh is None
        films = [plain, make_film(name, sky, mesh=None), make_film(name, sky, mesh=empty), make_film(name, sky)]
        for film in films:
            film.render(2), film.render_adaptive(2, 0.3, 8), film.render(2)
        want = films[0].state()
        assert films[1].state() == want and films[2].state() == want
        assert films[3].state()[88:] != want[88:]
        got = films[3].image(out_f64=True)
        assert np.isfinite(got).all() and (bits(got) != bits(films[0].image(out_f64=True))).any(axis=2).sum() >= 10, sky
        for film in films:
            film.close()
    empty.close()


# ---- 6. readers on the records

@pytest.mark.parametrize("name,sky", [("room", True), ("mesh1", False)])
def test_noise_filter_and_history_read_the_records(name, sky):
    rgb, q = reading(name, sky, False)
    frame, s1, s2, m = _film.expectation(rgb, FM.C, 6)
    film = make_film(name, sky)
    film.render(2), film.render(4)
    before = film.state()
    plane = G.noise_plane(s1, s2, np.full((2, 3), 6), FM.C)
    assert same(film.noise(), plane)
    color, noise, feats = film.image(out_f64=True), film.noise(), film.features()
    sigmas = dict(sigma_normal=0.5, sigma_albedo=0.2, sigma_depth=2.0, sigma_luminance=4.0)
    want = rayrs_amd.denoise_guided(color, noise, feats["normal"], feats["albedo"], feats["depth"], levels=2, **sigmas)
    got = film.denoised_guided(levels=2, out_f64=True, **sigmas)
    assert same(got, want) and not same(got, color)
    plain = dict(sigma_normal=0.5, sigma_albedo=0.2, sigma_depth=2.0, sigma_color=4.0)
    assert same(film.denoised(levels=2, out_f64=True, **plain),
                rayrs_amd.denoise(color, feats["normal"], feats["albedo"], feats["depth"], levels=2, **plain))
    cam = camera_of(name)
    a, b = rayrs_amd.History(), rayrs_amd.History()
    a.push(film)
    b.push_image(cam, color, noise, np.full((FM.H, FM.W), 6.0), feats["normal"], feats["albedo"], feats["depth"], feats["coverage"], feats["object"])
    for x, y in zip(a.read(), b.read()):
        assert same(x, y)
    assert same(film.image(out_f64=True), frame) and film.state() == before


def test_render_until_and_render_sequence_take_a_group_through_the_films_arguments():
    name, sky = "room", True
    rgb, q = reading(name, sky, False)
    tau = adaptive_tau(name, sky, False)[0]
    film, rep = make_film(name, sky), _film_adaptive.Replay(rgb, q, c=FM.C)
    st, reason = rayrs_amd.render_until(film, tau, pass_samples=2, max_samples=8, adaptive=True)
    passes, want_reason = _film_adaptive.replay_until(rep, tau=tau, step=2, cap=8)
    assert reason == want_reason and np.array_equal(film.tile_samples(), rep.nt) and same(film.image(out_f64=True), rep.frame())
    f = fam(name)
    seq = list(rayrs_amd.render_sequence(f.scene, [camera_of(name)], 4, sample_chunk=FM.C, seed=FM.SEED, lights=FM.lights(name, sky), direct=True,
                                         mesh=f.mesh))
    assert len(seq) == 1 and seq[0][0].mesh is f.mesh
    assert same(seq[0][0].image(out_f64=True), _film.expectation(rgb, FM.C, 4)[0])
    lone = make_film(name, sky)
    lone.render(4)
    hist = rayrs_amd.History()
    hist.push(lone)
    for x, y in zip(seq[0][1].read(), hist.read()):
        assert same(x, y)


# ---- 7. the pass limit

def test_a_pass_longer_than_one_launch_per_tile_is_refused_and_leaves_the_film():
    film = make_film("room", True)
    film.render(2)
    before = film.state()
    for call in (lambda: film.render(2 * 16385), lambda: film.render_adaptive(2 * 16385, 0.1)):
        with pytest.raises(_ffi.RayrsError) as e:
            call()
        assert e.value.status == UNSUPPORTED
    assert film.state() == before


# ---- 8. neighbours

def test_the_neighbours_on_the_shared_scratch_keep_their_bits():
    name = "mesh1"
    f = fam(name)
    cam = camera_of(name)
    lamps = FM.lights(name, False)

    def neighbours():
        plain = rayrs_amd.Film(f.scene, cam, sample_chunk=FM.C, seed=FM.SEED)
        plain.render(4)
        return (plain.state(), rayrs_amd.render(f.scene, cam, spp=4, seed=FM.SEED, out_f64=True)[0],
                rayrs_amd.render_lit(f.scene, cam, 4, lamps, seed=FM.SEED, sample_chunk=2, direct=True),
                rayrs_amd.render_lit(f.scene, cam, 4, lamps, seed=FM.SEED, sample_chunk=2, direct=True, mesh=f.mesh),
                f.scene.radiance(f.o, f.d, samples=3, seed=FM.SEED, lights=lamps + [SKY], direct=True, mesh=f.mesh))
    before = neighbours()
    for sky in (False, True):
        for fast in (False, True):
            film = make_film(name, sky, fast)
            film.render(2), film.render_adaptive(2, 0.1, 8), film.render(2)
    after = neighbours()
    assert before[0] == after[0]
    for x, y in zip(before[1:], after[1:]):
        assert same(x, y)


# ---- 9. the large frame: two launches a pass, an accumulate per tile range

BIG_W, BIG_H, BIG_C = 472, 456, 4


@pytest.mark.parametrize("sky", [False, True])
def test_a_pass_of_two_launches_is_the_image_forms_frame(sky):
    assert ((BIG_W + 7) // 8) * ((BIG_H + 7) // 8) * 64 * 5 > 1 << 20
    f = fam("mesh1")
    cam = rayrs_amd.Camera(*scenes.camera_for_resolution(mesh1_objects()[0], BIG_W, BIG_H))
    lights = FM.lights("mesh1", sky)
    img, cnt = rayrs_amd.render_lit(f.scene, cam, 20, lights, seed=FM.SEED, sample_chunk=BIG_C, queries=True, direct=True, mesh=f.mesh)
    assert np.isfinite(img).all()
    for parts in ((20,), (8, 12)):
        film = rayrs_amd.Film(f.scene, cam, sample_chunk=BIG_C, seed=FM.SEED, lights=lights, direct=True, mesh=f.mesh)
        for n in parts:
            film.render(n)
        assert same(film.image(out_f64=True), img), (sky, parts)
        st = film.status(0.2)
        assert st["rays"] == int(cnt.sum(dtype=np.uint64)) and st["paths"] == BIG_W * BIG_H * 20, (sky, parts, st)
        film.close()
