"""The mesh-lit bakes (include/rayrs_hip.h MESH-LIT FILMS AND BAKES) on the GPU, bit for bit and count for count.

With 1 to 130 points in chunks of 2 the expectation is the plain-Python reading's per-sample values (tests/_film_mesh.py over
tests/_mesh.py), folded by tests/_bake.py's Replay, each point at its own sample count: nothing in it calls the library, and every
expected value is finite, so each comparison is of bits.  The families are tests/test_gpu_mesh_lights.py's `room` and `mesh1`
(on both walks), each kind without and with the sky.

At 2^19 + 65 points in chunks of 2 -- a pass of 4 samples is two chunks per point, the items past 2^20: two launches -- there is no
Python reading: the reference is scene.irradiance(mesh=group), which tests/test_gpu_mesh_lights.py holds to the reading."""
import functools

import numpy as np
import pytest

import _bake as B
import _film_mesh as FM
import rayrs_amd
from rayrs_amd import _ffi
from test_gpu_film_mesh import bits, fam, same

pytestmark = pytest.mark.gpu

WALKS = [("room", False), ("mesh1", False), ("mesh1", True)]
KINDS = ("irradiance", "radiance")
CASES = [(name, fast, kind, sky) for name, fast in WALKS for kind in KINDS for sky in (False, True)]
INVALID_ARG = -1
HEADER = 96   # bytes of a checkpoint image before the records
N = FM.N_POINTS


def make_bake(name, kind, sky, fast=False, lo=0, hi=N, mesh="group", **kw):
    f = fam(name)
    a, b = FM.inputs(name, kind)
    settings = dict(kind=kind, sample_chunk=FM.C, max_bounces=FM.BOUNCES, seed=FM.SEED, bias=FM.BIAS, fast_traversal=fast,
                    lights=FM.lights(name, sky), direct=True, mesh=f.mesh if mesh == "group" else mesh)
    settings.update(kw)
    return rayrs_amd.Bake(f.scene, a[lo:hi], b[lo:hi], **settings)


def reading(name, kind, sky, fast=False):
    fam(name)   # (registers the reading that walks the product's fast tree)
    values, q = FM.point_paths(name, kind, sky, fast)
    assert values.shape == (N, FM.N_MAX, 3) and np.isfinite(values).all()
    return values, q


def check(bake, rep, what):
    """The bake's values, queries, counts, status over the tau grid and noise are the replay's."""
    values, queries = bake.values(queries=True)
    assert np.isfinite(rep.values()).all() and same(values, rep.values()), what
    assert queries.dtype == np.uint64 and np.array_equal(queries, rep.queries()), what
    assert np.array_equal(bake.point_samples(), rep.ni), what
    for tau in B.TAUS:
        st = bake.status(tau)
        assert (st["unconverged"], st["nonfinite"]) == rep.counts(tau), (what, tau, st)
        assert (st["samples"], st["points"], st["closed"]) == (int(rep.ni.max(initial=0)), rep.n, int(rep.closed)), (what, st)
        assert (st["rays"], st["paths"]) == (rep.rays, rep.paths), (what, st)
    assert same(bake.noise(), rep.noise()), what


# ---- 1. the contract

@pytest.mark.parametrize("name,fast,kind,sky", CASES)
def test_passes_and_status_are_the_readings(name, fast, kind, sky):
    values, q = reading(name, kind, sky, fast)
    for n_points in FM.SIZES:
        bake = make_bake(name, kind, sky, fast, hi=n_points)
        assert bake.mesh is fam(name).mesh and bake.lights == FM.lights(name, sky)
        rep = B.Replay(values, q, c=FM.C, n_points=n_points)
        for step in (2, 4, 3):
            st = bake.render(step)
            want = rep.uniform_pass(step)
            assert (st["points"], st["paths"], st["rays"], st["launches"]) == (n_points, n_points * step, want["rays"], 1), (n_points, step, st)
            check(bake, rep, (name, fast, kind, sky, n_points, step))
        before = bake.state()
        for call in (lambda: bake.render(2), lambda: bake.render_adaptive(2, 0.1)):   # the pass of 3 closed the bake
            with pytest.raises(_ffi.RayrsError) as e:
                call()
            assert e.value.status == INVALID_ARG
        assert bake.state() == before
        bake.close()


# ---- 2. partitions, and a checkpoint into a new bake

PARTITIONS = ((8,), (2, 6), (6, 2), (4, 4), (2, 2, 4), (2, 2, 2, 2))


@pytest.mark.parametrize("name,kind,sky", [("room", "irradiance", True), ("mesh1", "radiance", False), ("mesh1", "irradiance", True)])
def test_partitions_and_a_checkpoint_leave_the_same_bits(name, kind, sky, tmp_path):
    states = []
    for parts in PARTITIONS:
        bake = make_bake(name, kind, sky)
        for n in parts:
            bake.render(n)
        states.append(bake.state())
    assert len(states[0]) == HEADER + N * (5 * 8 + 8 + 4)
    assert all(s == states[0] for s in states[1:])
    values, q = reading(name, kind, sky)
    rep = B.Replay(values, q, c=FM.C)
    rep.uniform_pass(8)
    for cut in (2, 6):
        first = make_bake(name, kind, sky)
        first.render(cut)
        first.save(tmp_path / "bake.state")
        second = make_bake(name, kind, sky)
        second.load(tmp_path / "bake.state")
        second.render(8 - cut)
        assert second.state() == states[0], cut
        check(second, rep, (name, kind, sky, cut))


# ---- 3. adaptive passes against the replay

SEQUENCE = ("adaptive", "uniform", "adaptive", "adaptive")   # passes of 2 under a cap of 8
TAU_GRID = tuple(float(t) for t in np.round(np.geomspace(0.02, 0.9, 24), 3)) + (0.95, 0.98, 0.99)
QUARTER = -(-N // 4)


def replay_sequence(values, q, tau):
    rep, out = B.Replay(values, q, c=FM.C), []
    for kind in SEQUENCE:
        want = rep.adaptive_pass(2, tau, 8) if kind == "adaptive" else rep.uniform_pass(2)
        out.append((kind, want, rep.counts(tau), rep.rays, rep.paths))
    return rep, out


@functools.lru_cache(maxsize=None)
def adaptive_tau(name, fast, kind, sky):
    """The first tau of TAU_GRID, chosen from the reading alone, at which some adaptive pass of SEQUENCE takes at least a quarter of
    the points and leaves at least a quarter; None where the reading has none.  (On the default walk's readings these are taus of
    0.172 to 0.283, whose second adaptive pass takes 97 to 104 of the 130 points.)"""
    values, q = reading(name, kind, sky, fast)
    for tau in TAU_GRID:
        if any(kind_ == "adaptive" and QUARTER <= want["points"] <= N - QUARTER for kind_, want, *_ in replay_sequence(values, q, tau)[1]):
            return tau
    return None


@pytest.mark.parametrize("name,fast,kind,sky", CASES)
def test_adaptive_passes_are_the_replay(name, fast, kind, sky):
    values, q = reading(name, kind, sky, fast)
    tau = adaptive_tau(name, fast, kind, sky)
    assert tau is not None, "no tau of the grid splits the points: the points are wrong, not the condition"
    bake = make_bake(name, kind, sky, fast)
    split = False
    for kind_, want, counts, rays, paths in replay_sequence(values, q, tau)[1]:
        ni_before = bake.point_samples()
        got_before, q_before = bake.values(queries=True)
        if kind_ == "adaptive":
            active, st = bake.render_adaptive(2, tau, 8)
            assert active == want["points"], (kind_, active, want["points"])
            split = split or QUARTER <= active <= N - QUARTER
        else:
            st = bake.render(2)
        assert (st["points"], st["rays"], st["paths"]) == (want["points"], want["rays"], want["paths"]), (kind_, st)
        assert np.array_equal(bake.point_samples(), want["ni"]), kind_
        # the pass took the replay's points -- the list is ascending, so its launch's entries are they in order -- and no other
        taken = np.flatnonzero(bake.point_samples() != ni_before)
        assert np.array_equal(taken, np.flatnonzero(want["active"])) and (np.diff(taken) > 0).all(), kind_
        got, got_q = bake.values(queries=True)
        assert same(got, want["values"]) and np.array_equal(got_q, want["queries"]), kind_
        out = ~want["active"]   # a point that stays out keeps its bits
        assert np.array_equal(bits(got)[out], bits(got_before)[out]) and np.array_equal(got_q[out], q_before[out]), kind_
        status = bake.status(tau)
        assert (status["unconverged"], status["nonfinite"], status["rays"], status["paths"]) == (*counts, rays, paths), (kind_, status)
        assert status["samples"] == int(want["ni"].max())
    assert split
    rep = replay_sequence(values, q, tau)[0]
    check(bake, rep, (name, fast, kind, sky, tau))
    assert len(np.unique(rep.ni)) > 1


def test_bake_until_is_the_replays_loop():
    name, kind, sky = "room", "irradiance", True
    values, q = reading(name, kind, sky)
    tau = adaptive_tau(name, False, kind, sky)
    for adaptive in (True, False):
        bake, rep = make_bake(name, kind, sky), B.Replay(values, q, c=FM.C)
        st, reason = rayrs_amd.bake_until(bake, tau, pass_samples=1, max_samples=8, adaptive=adaptive)   # (a pass of 1 is rounded up to c)
        while True:
            if int(rep.ni.max()) > 0 and rep.counts(tau)[0] == 0:
                want = "converged"
                break
            if not adaptive and int(rep.ni.max()) + 2 > 8:
                want = "max_samples"
                break
            if adaptive:
                if rep.adaptive_pass(2, tau, 8)["points"] == 0:
                    want = "max_samples"
                    break
            else:
                rep.uniform_pass(2)
        assert reason == want and st["point_samples"] == int(rep.ni.sum()) and st["unconverged"] == rep.counts(tau)[0], (adaptive, st, reason)
        check(bake, rep, adaptive)


# ---- 4. a slice with index_base

@pytest.mark.parametrize("name,kind,sky,fast", [("room", "irradiance", False, False), ("mesh1", "radiance", True, True)])
def test_a_slice_with_its_index_base_is_the_slice_of_the_whole_bake(name, kind, sky, fast):
    whole = make_bake(name, kind, sky, fast)
    whole.render(2), whole.render(4)
    values, queries = whole.values(queries=True)
    want = B.Replay(*reading(name, kind, sky, fast), c=FM.C)
    want.uniform_pass(6)
    assert same(values, want.values()) and np.array_equal(queries, want.queries())
    part = make_bake(name, kind, sky, fast, lo=40, hi=100, index_base=40)
    part.render(4), part.render(2)
    got, got_q = part.values(queries=True)
    assert same(got, values[40:100]) and np.array_equal(got_q, queries[40:100])
    assert same(part.noise(), whole.noise()[40:100])
    shifted = make_bake(name, kind, sky, fast, lo=40, hi=100)   # (not vacuous: without its index_base the slice has other bits)
    shifted.render(6)
    assert (bits(shifted.values()) != bits(values[40:100])).any(axis=1).sum() >= 10


# ---- 5. the empty group

@pytest.mark.parametrize("name,kind", [("room", "irradiance"), ("mesh1", "radiance")])
def test_an_empty_group_is_the_bake_of_the_list_and_a_group_is_not(name, kind):
    f = fam(name)
    a, b = FM.inputs(name, kind)
    empty = f.scene.mesh_lights([])
    for sky in (False, True):
        settings = dict(kind=kind, sample_chunk=FM.C, max_bounces=FM.BOUNCES, seed=FM.SEED, bias=FM.BIAS, lights=FM.lights(name, sky), direct=True)
        plain = rayrs_amd.Bake(f.scene, a, b, **settings)
        assert plain.mesh is None
        bakes = [plain, rayrs_amd.Bake(f.scene, a, b, mesh=None, **settings), make_bake(name, kind, sky, mesh=empty), make_bake(name, kind, sky)]
        for bake in bakes:
            bake.render(2), bake.render_adaptive(2, 0.3, 8), bake.render(2)
        want = bakes[0].state()
        assert bakes[1].state() == want and bakes[2].state() == want
        assert bakes[3].state()[HEADER:] != want[HEADER:]
        values = bakes[3].values()
        # (not vacuous: the group changes the bits of the points whose paths credit a light sample -- on mesh1's rays a handful)
        assert np.isfinite(values).all() and (bits(values) != bits(bakes[0].values())).any(), sky
        for bake in bakes:
            bake.close()
    # without a list and without a sky the empty group's bake is the unlit one
    none = dict(kind=kind, sample_chunk=FM.C, max_bounces=FM.BOUNCES, seed=FM.SEED, bias=FM.BIAS)
    unlit, grouped = rayrs_amd.Bake(f.scene, a, b, **none), rayrs_amd.Bake(f.scene, a, b, lights=[], direct=True, mesh=empty, **none)
    for bake in (unlit, grouped):
        bake.render(2), bake.render(4)
    assert grouped.state() == unlit.state()
    unlit.close(), grouped.close()
    empty.close()


def test_closing_after_the_scene_calls_nothing_of_the_library():
    """The header's rule is that the scene outlives its films, bakes and groups.  Python cannot promise that order where it
    finalizes garbage -- at interpreter exit a scene and its dependents go in any order -- so a dependent whose scene is already
    closed drops its handle without a call: the library's destructors would read the freed scene."""
    import _mesh
    from test_gpu_mesh_lights import HDRI, Z_FAR, Z_NEAR
    cam_args, objs, heur, names = _mesh.mesh_room(small=True)
    scene = rayrs_amd.Scene(objs, Z_NEAR, Z_FAR, heur, HDRI, device=0)
    group = scene.mesh_lights(names["group"])
    p = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 1.0]])
    nrm = np.tile((0.0, 1.0, 0.0), (2, 1))
    bake = rayrs_amd.Bake(scene, p, nrm, sample_chunk=2, lights=[], direct=True, mesh=group)
    film = rayrs_amd.Film(scene, rayrs_amd.Camera(*FM.description("small")[0]), sample_chunk=2, lights=[], direct=True, mesh=group)
    bake.render(2), film.render(2)   # (the group's table is on the device now)
    assert np.isfinite(bake.values()).all() and np.isfinite(film.image(out_f64=True)).all()
    scene.close()
    for dependent in (film, bake, group):
        dependent.close()
        assert dependent._h is None


# ---- 6. at size: two launches a pass

BIG_N = (1 << 19) + 65


@functools.lru_cache(maxsize=None)
def big_inputs():
    """A floor grid of 1024 points a row under mesh1's lamp and mesh, normals up, every third normal NaN."""
    index = np.arange(BIG_N)
    p = np.stack([-4.0 + 8.0 * (index % 1024) / 1023.0, np.zeros(BIG_N), -4.0 + 8.0 * (index // 1024) / 512.0], axis=1)
    nrm = np.tile((0.0, 1.0, 0.0), (BIG_N, 1))
    nrm[index % 3 == 0] = np.nan
    p.setflags(write=False), nrm.setflags(write=False)
    return p, nrm


@pytest.mark.parametrize("sky", [False, True])
def test_at_size_a_pass_of_two_launches_is_the_querys_answer(sky):
    assert BIG_N * 2 > 1 << 20
    f = fam("mesh1")
    p, nrm = big_inputs()
    lights = FM.lights("mesh1", sky)
    rad, cnt = f.scene.irradiance(p, nrm, samples=4, bias=FM.BIAS, max_bounces=FM.BOUNCES, seed=FM.SEED, sample_chunk=2, queries=True, lights=lights,
                                  direct=True, mesh=f.mesh)
    good = np.arange(BIG_N) % 3 != 0
    assert np.isfinite(rad[good]).all() and (rad[good] > 0.0).any(axis=1).mean() > 0.5
    bake = rayrs_amd.Bake(f.scene, p, nrm, sample_chunk=2, max_bounces=FM.BOUNCES, seed=FM.SEED, bias=FM.BIAS, lights=lights, direct=True, mesh=f.mesh)
    st = bake.render(4)
    assert (st["points"], st["paths"], st["launches"]) == (BIG_N, BIG_N * 4, 2) and st["rays"] == int(cnt.sum(dtype=np.uint64)), st
    values, queries = bake.values(queries=True)
    assert same(values, rad) and np.array_equal(queries, cnt.astype(np.uint64))
    assert (bake.point_samples() == 4).all()
    bake.close()
