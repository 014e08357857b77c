"""The bake (include/rayrs_hip.h BAKE) on the GPU, bit for bit and count for count.

With 1 to 130 points in chunks of 2 the expectation is the plain-Python readings' per-sample values (tests/_bake.py), folded by
_film.expectation and _film.noise_masks, each point at its own sample count, and by the replay of SELECTION: nothing in it calls
the library.  The families are tests/_film_direct.py's `room` under the studio map with its two lamps and `mesh1_light` under the
gradient map with its lamp (streams, hot group, a fast walk of its own), each as an unlit, a direct-lit and a sky bake of either
kind, the mesh scene on both walks.

At 2^20 + 65 points in chunks of 1 -- the smallest bake whose pass needs two launches and whose selection scans more workgroup
counts than one step of the scan holds -- there is no Python reading: the reference is scene.irradiance, which
tests/test_gpu_radiance.py holds to the readings."""
import functools

import numpy as np
import pytest

import _bake as B
import _film_direct as FD
import rayrs_amd
from rayrs_amd import _ffi
from test_gpu_film_direct import camera_of, scene_of

pytestmark = pytest.mark.gpu

WALKS = [("room", False), ("mesh1_light", False), ("mesh1_light", True)]
CASES = [(name, fast, strategy, kind) for name, fast in WALKS for strategy in B.STRATEGIES for kind in B.KINDS]
INVALID_ARG, UNSUPPORTED = -1, -5
HEADER = 96   # bytes of a checkpoint image before the records


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64 if np.asarray(x).dtype == np.float64 else np.uint32)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def make_bake(name, strategy, kind, fast=False, lo=0, hi=B.N_POINTS, **kw):
    a, b = B.inputs(name, kind)
    settings = dict(kind=kind, sample_chunk=B.C, max_bounces=B.BOUNCES, seed=B.SEED, bias=B.BIAS, fast_traversal=fast)
    settings.update(B.lights(name, strategy))
    settings.update(kw)
    return rayrs_amd.Bake(scene_of(name), a[lo:hi], b[lo:hi], **settings)


def reading(name, strategy, kind, fast=False):
    scene_of(name)   # (registers the oracle that walks the product's fast tree)
    return B.paths(name, strategy, kind, fast)


def check(bake, rep, what):
    """The bake's values, queries, counts, status over the tau grid and noise are the replay's."""
    values, queries = bake.values(queries=True)
    assert same(values, rep.values()), what
    assert queries.dtype == np.uint64 and np.array_equal(queries, rep.queries()), what
    assert np.array_equal(bake.point_samples(), rep.ni), what
    for tau in B.TAUS:
        st = bake.status(tau)
        assert (st["unconverged"], st["nonfinite"]) == rep.counts(tau), (what, tau, st)
        assert (st["samples"], st["points"], st["closed"]) == (int(rep.ni.max(initial=0)), rep.n, int(rep.closed)), (what, st)
        assert (st["rays"], st["paths"]) == (rep.rays, rep.paths), (what, st)
    assert same(bake.noise(), rep.noise()), what


# ---- 1. passes and status

@pytest.mark.parametrize("name,fast,strategy,kind", CASES)
def test_passes_and_status_are_the_readings(name, fast, strategy, kind):
    values, q = reading(name, strategy, kind, fast)
    assert np.isfinite(values).all()
    for n_points in B.SIZES:
        bake = make_bake(name, strategy, kind, fast, hi=n_points)
        rep = B.Replay(values, q, n_points=n_points)
        for step in (2, 4, 3):
            st = bake.render(step)
            want = rep.uniform_pass(step)
            assert (st["points"], st["paths"], st["rays"], st["launches"]) == (n_points, n_points * step, want["rays"], 1), (n_points, step, st)
            check(bake, rep, (name, fast, strategy, kind, n_points, step))
        before = bake.state()
        for call in (lambda: bake.render(2), lambda: bake.render_adaptive(2, 0.1)):   # the pass of 3 closed the bake
            with pytest.raises(_ffi.RayrsError) as e:
                call()
            assert e.value.status == INVALID_ARG
        with pytest.raises(_ffi.RayrsError) as e:
            bake.render(0)
        assert e.value.status == INVALID_ARG
        assert bake.state() == before
        bake.close()


def test_a_pass_of_more_than_65536_chunks_is_refused_and_leaves_the_bake():
    bake = make_bake("room", "sky", "irradiance", hi=3)
    bake.render(2)
    before = bake.state()
    for call in (lambda: bake.render(2 * 65537), lambda: bake.render_adaptive(2 * 65537, 0.1), lambda: bake.render(1 << 30)):
        with pytest.raises(_ffi.RayrsError) as e:
            call()
        assert e.value.status == UNSUPPORTED
    for call in (lambda: bake.render_adaptive(3, 0.1), lambda: bake.render_adaptive(2, -0.1), lambda: bake.render_adaptive(2, float("nan"))):
        with pytest.raises(_ffi.RayrsError) as e:
            call()
        assert e.value.status == INVALID_ARG
    assert bake.state() == before


# ---- 2. partitions and checkpoint

PARTITIONS = ((8,), (2, 6), (6, 2), (4, 4), (2, 2, 4), (2, 4, 2), (4, 2, 2), (2, 2, 2, 2))


@pytest.mark.parametrize("name,strategy,kind", [("room", "sky", "irradiance"), ("mesh1_light", "direct", "radiance"),
                                                ("mesh1_light", "unlit", "irradiance")])
def test_partitions_and_a_checkpoint_leave_the_same_bits(name, strategy, kind, tmp_path):
    states = []
    for parts in PARTITIONS:
        bake = make_bake(name, strategy, kind)
        for n in parts:
            bake.render(n)
        states.append(bake.state())
    assert len(states[0]) == HEADER + B.N_POINTS * (5 * 8 + 8 + 4)
    assert all(s == states[0] for s in states[1:])
    values, q = reading(name, strategy, kind)
    rep = B.Replay(values, q)
    rep.uniform_pass(8)
    for cut in (2, 4, 6):
        first = make_bake(name, strategy, kind)
        first.render(cut)
        first.save(tmp_path / "bake.state")
        second = make_bake(name, strategy, kind)
        second.load(tmp_path / "bake.state")
        second.render(8 - cut)
        assert second.state() == states[0], cut
        check(second, rep, (name, strategy, kind, cut))


def test_state_set_refuses_another_bakes_image():
    bake = make_bake("room", "direct", "irradiance", hi=65)
    bake.render(2)
    image = bake.state()
    others = (dict(sample_chunk=4), dict(seed=B.SEED + 1), dict(max_bounces=7), dict(index_base=1), dict(bias=2e-4), dict(fast_traversal=True),
              dict(hi=64), dict(radiance=True), dict(lights=list(B.lights("room", "sky")["lights"])))
    for other in others:
        other = dict(other)
        kind = "radiance" if other.pop("radiance", False) else "irradiance"
        b2 = make_bake("room", "direct", kind, **{"hi": 65, **other})
        empty = b2.state()
        with pytest.raises(_ffi.RayrsError) as e:
            b2.set_state(image)
        assert e.value.status == INVALID_ARG, other
        assert b2.state() == empty, other
    twin = make_bake("room", "direct", "irradiance", hi=65)
    empty = twin.state()
    bad_version = image[:4] + (2).to_bytes(4, "little") + image[8:]
    # counts that no sequence of passes leaves: an odd count in an open bake of chunks of 2, and a largest count that is not the header's
    odd_count = image[:-4] + (3).to_bytes(4, "little")
    high_count = image[:-4] + (4).to_bytes(4, "little")
    for bad in (image[:-1], image + b"\0", image[:HEADER - 8], bad_version, b"\0" * len(image), odd_count, high_count):
        with pytest.raises(_ffi.RayrsError) as e:
            twin.set_state(bad)
        assert e.value.status == INVALID_ARG
        assert twin.state() == empty
    # (the list is not recorded: a bake with the same settings and another list takes the image, as a film does)
    twin.set_state(image)
    assert twin.state() == image
    relit = make_bake("room", "direct", "irradiance", hi=65, lights=[B.lights("room", "direct")["lights"][0]])
    relit.set_state(image)
    assert relit.state() == image


# ---- 3. adaptive passes

SEQUENCE = ("adaptive", "uniform", "adaptive", "adaptive")   # passes of 2 under a cap of 8
TAU_GRID = tuple(float(t) for t in np.round(np.geomspace(0.02, 0.9, 24), 3)) + (0.95, 0.98, 0.99)
QUARTER = -(-B.N_POINTS // 4)


def replay_sequence(values, q, tau):
    rep, out = B.Replay(values, q), []
    for kind in SEQUENCE:
        want = rep.adaptive_pass(2, tau, 8) if kind == "adaptive" else rep.uniform_pass(2)
        out.append((kind, want, rep.counts(tau), rep.rays, rep.paths))
    return rep, out


@functools.lru_cache(maxsize=None)
def adaptive_tau(name, fast, strategy, kind):
    """The first tau of TAU_GRID, chosen from the reading alone, at which some adaptive pass of SEQUENCE takes at least a quarter of
    the points and leaves at least a quarter; None where the reading has none."""
    values, q = reading(name, strategy, kind, fast)
    for tau in TAU_GRID:
        if any(kind_ == "adaptive" and QUARTER <= want["points"] <= B.N_POINTS - QUARTER for kind_, want, *_ in replay_sequence(values, q, tau)[1]):
            return tau
    return None


@pytest.mark.parametrize("name,fast,strategy,kind", CASES)
def test_adaptive_passes_are_the_replay(name, fast, strategy, kind):
    values, q = reading(name, strategy, kind, fast)
    tau = adaptive_tau(name, fast, strategy, kind)
    assert tau is not None, "no tau of the grid splits the points: the points are wrong, not the condition"
    bake = make_bake(name, strategy, kind, fast)
    split = False
    for kind_, want, counts, rays, paths in replay_sequence(values, q, tau)[1]:
        if kind_ == "adaptive":
            active, st = bake.render_adaptive(2, tau, 8)
            assert active == want["points"], (kind_, active, want["points"])
            split = split or QUARTER <= active <= B.N_POINTS - QUARTER
        else:
            st = bake.render(2)
        assert (st["points"], st["rays"], st["paths"]) == (want["points"], want["rays"], want["paths"]), (kind_, st)
        assert np.array_equal(bake.point_samples(), want["ni"]), kind_
        got, got_q = bake.values(queries=True)
        assert same(got, want["values"]) and np.array_equal(got_q, want["queries"]), kind_
        status = bake.status(tau)
        assert (status["unconverged"], status["nonfinite"], status["rays"], status["paths"]) == (*counts, rays, paths), (kind_, status)
        assert status["samples"] == int(want["ni"].max())
    assert split
    rep = replay_sequence(values, q, tau)[0]
    check(bake, rep, (name, fast, strategy, kind, tau))
    assert len(np.unique(rep.ni)) > 1
    # every point has its cap or is converged: a further pass takes those below the cap that are still noisy, then none
    while True:
        want = rep.adaptive_pass(2, tau, 8)
        active, st = bake.render_adaptive(2, tau, 8)
        assert active == want["points"]
        if active == 0:
            assert (st["points"], st["rays"], st["paths"], st["launches"]) == (0, 0, 0, 0)
            break
    check(bake, rep, (name, fast, strategy, kind, tau, "end"))


def test_bake_until_is_the_replays_loop():
    name, strategy, kind = "room", "direct", "irradiance"
    values, q = reading(name, strategy, kind)
    tau = adaptive_tau(name, False, strategy, kind)
    for adaptive in (True, False):
        bake, rep = make_bake(name, strategy, kind), B.Replay(values, q)
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


# ---- 4. the empty list

@pytest.mark.parametrize("name,kind", [("room", "irradiance"), ("mesh1_light", "irradiance"), ("mesh1_light", "radiance")])
def test_an_empty_list_is_the_unlit_bake_and_a_list_is_not(name, kind):
    scene = scene_of(name)
    a, b = B.inputs(name, kind)
    unlit, empty = make_bake(name, "unlit", kind), make_bake(name, "unlit", kind, lights=[], direct=True)
    for bake in (unlit, empty):
        bake.render(2), bake.render(4)
    assert empty.state() == unlit.state()
    query = scene.irradiance if kind == "irradiance" else scene.radiance
    kw = dict(bias=B.BIAS) if kind == "irradiance" else {}
    rad, cnt = query(a, b, samples=6, max_bounces=B.BOUNCES, seed=B.SEED, sample_chunk=B.C, queries=True, **kw)
    got, got_q = empty.values(queries=True)
    assert same(got, rad) and np.array_equal(got_q, cnt.astype(np.uint64))
    for strategy in ("direct", "sky"):
        lit = make_bake(name, strategy, kind)
        lit.render(2), lit.render(4)
        values = lit.values()
        assert np.isfinite(values).all() and (bits(values) != bits(rad)).any(axis=1).sum() >= 10, strategy
        rad_lit, cnt_lit = query(a, b, samples=6, max_bounces=B.BOUNCES, seed=B.SEED, sample_chunk=B.C, queries=True, **kw, **B.lights(name, strategy))
        assert same(values, rad_lit) and np.array_equal(lit.values(queries=True)[1], cnt_lit.astype(np.uint64)), strategy


# ---- 5. index_base

@pytest.mark.parametrize("name,strategy,kind", [("room", "direct", "irradiance"), ("mesh1_light", "sky", "radiance")])
def test_a_slice_with_its_index_base_is_the_slice_of_the_whole_bake(name, strategy, kind):
    whole = make_bake(name, strategy, kind)
    whole.render(2), whole.render(4)
    values, queries = whole.values(queries=True)
    for lo, hi in ((40, 107), (0, 64), (129, 130)):
        part = make_bake(name, strategy, kind, lo=lo, hi=hi, index_base=lo)
        part.render(4), part.render(2)
        got, got_q = part.values(queries=True)
        assert same(got, values[lo:hi]) and np.array_equal(got_q, queries[lo:hi]), (lo, hi)
        assert same(part.noise(), whole.noise()[lo:hi])
    shifted = make_bake(name, strategy, kind, lo=40, hi=107)
    shifted.render(6)
    assert (bits(shifted.values()) != bits(values[40:107])).any(axis=1).sum() >= 10
    # ... and the whole bake with an index_base is the reading's with that index_base
    based = make_bake(name, strategy, kind, lo=0, hi=5, index_base=1 << 40)
    based.render(6)
    a, b = B.inputs(name, kind)
    scene = scene_of(name)
    query = scene.irradiance if kind == "irradiance" else scene.radiance
    kw = dict(bias=B.BIAS) if kind == "irradiance" else {}
    rad = query(a[:5], b[:5], samples=6, max_bounces=B.BOUNCES, seed=B.SEED, sample_chunk=B.C, index_base=1 << 40, **kw, **B.lights(name, strategy))
    assert same(based.values(), rad)


# ---- 6. neighbours unharmed

def test_the_neighbours_on_the_shared_scratch_keep_their_bits():
    name = "mesh1_light"
    scene, cam = scene_of(name), camera_of(name)
    p, nrm = B.inputs(name, "irradiance")
    lamps = FD.lights(name, "direct")

    def neighbours():
        film = rayrs_amd.Film(scene, cam, sample_chunk=FD.C, seed=FD.SEED, lights=lamps, direct=True)
        film.render(4)
        rad, cnt = scene.irradiance(p, nrm, samples=3, bias=B.BIAS, seed=B.SEED, queries=True)
        return film.state(), rad, cnt
    before = neighbours()
    bakes = [make_bake(name, strategy, "irradiance") for strategy in B.STRATEGIES]
    for bake in bakes:
        bake.render(2)
    middle = neighbours()
    for bake in bakes:
        bake.render_adaptive(2, 0.1, 8), bake.render(2)
    after = neighbours()
    for other in (middle, after):
        assert before[0] == other[0]
        assert same(before[1], other[1]) and np.array_equal(before[2], other[2])
    # ... and the bakes kept theirs through the neighbours' launches
    for strategy, bake in zip(B.STRATEGIES, bakes):
        values, q = reading(name, strategy, "irradiance")
        rep = B.Replay(values, q)
        rep.uniform_pass(2), rep.adaptive_pass(2, 0.1, 8), rep.uniform_pass(2)
        check(bake, rep, strategy)


# ---- 7. the empty bake, and no bounces

def test_an_empty_bake_is_legal_and_no_bounces_read_zero():
    scene = scene_of("room")
    empty = rayrs_amd.Bake(scene, np.zeros((0, 3)), np.zeros((0, 3)), sample_chunk=B.C)
    st = empty.render(2)
    assert (st["points"], st["paths"], st["rays"], st["launches"]) == (0, 0, 0, 0)
    active, st = empty.render_adaptive(2, 0.1)
    assert active == 0 and st["points"] == 0
    values, queries = empty.values(queries=True)
    assert values.shape == (0, 3) and queries.shape == (0,) and empty.point_samples().shape == (0,) and empty.noise().shape == (0,)
    status = empty.status(0.1)
    assert (status["points"], status["samples"], status["unconverged"], status["nonfinite"], status["rays"], status["closed"]) == (0, 0, 0, 0, 0, 0)
    assert len(empty.state()) == HEADER
    other = rayrs_amd.Bake(scene, np.zeros((0, 3)), np.zeros((0, 3)), sample_chunk=B.C)
    other.set_state(empty.state())
    empty.render(3)
    assert empty.status(0.1)["closed"] == 1
    for strategy in B.STRATEGIES:
        for kind in B.KINDS:
            bake = make_bake("room", strategy, kind, max_bounces=0)
            for step in (2, 4):
                st = bake.render(step)
                assert (st["points"], st["paths"], st["rays"], st["launches"]) == (B.N_POINTS, B.N_POINTS * step, 0, 0), st
            active, st = bake.render_adaptive(2, 0.0)   # (all zeros: S1 = S2 = 0 is converged at every tau with two chunks)
            assert active == 0
            values, queries = bake.values(queries=True)
            assert (bits(values) == 0).all() and (queries == 0).all() and (bake.point_samples() == 6).all()
            assert (bake.noise() == 0.0).all()
            status = bake.status(0.0)
            assert (status["unconverged"], status["nonfinite"], status["rays"], status["paths"]) == (0, 0, 0, 6 * B.N_POINTS)


# ---- 8. at size: two launches a pass, a scan of more workgroup counts than one step holds

BIG_N = (1 << 20) + 65


@functools.lru_cache(maxsize=None)
def big_inputs():
    """mesh1_light's 130 points tiled over 2^20 + 65, every third with a NaN normal, and two runs of 4000 and of 300 with one: whole
    workgroups of the select with nothing to take, and one that begins and ends inside a wave."""
    p, nrm = B.inputs("mesh1_light", "irradiance")
    index = np.arange(BIG_N)
    p, nrm = p[index % B.N_POINTS].copy(), nrm[index % B.N_POINTS].copy()
    bad = (index % 3 == 0) | ((index >= 5000) & (index < 9000)) | ((index >= (1 << 20) - 150) & (index < (1 << 20) + 150))
    nrm[bad] = np.nan
    p.setflags(write=False), nrm.setflags(write=False)
    return p, nrm


@functools.lru_cache(maxsize=None)
def big_reference(samples):
    p, nrm = big_inputs()
    rad, cnt = scene_of("mesh1_light").irradiance(p, nrm, samples=samples, bias=B.BIAS, max_bounces=B.BOUNCES, seed=B.SEED, sample_chunk=1,
                                                  queries=True)
    rad.setflags(write=False), cnt.setflags(write=False)
    return rad, cnt


def test_at_size_a_pass_of_two_launches_and_a_selection_of_many_workgroups():
    p, nrm = big_inputs()
    rad1, cnt1 = big_reference(1)
    finite = np.isfinite(rad1).all(axis=1)
    share = 1.0 - finite.mean()
    assert 0.25 <= share <= 0.75, share   # the points whose sample 0 is non-finite by scene.irradiance
    bake = rayrs_amd.Bake(scene_of("mesh1_light"), p, nrm, sample_chunk=1, max_bounces=B.BOUNCES, seed=B.SEED, bias=B.BIAS)
    st = bake.render(1)
    assert (st["points"], st["paths"], st["launches"]) == (BIG_N, BIG_N, 2) and st["rays"] == int(cnt1.sum(dtype=np.uint64)), st
    values1, queries1 = bake.values(queries=True)
    assert same(values1, rad1) and np.array_equal(queries1, cnt1.astype(np.uint64))
    status = bake.status(0.0)
    assert (status["unconverged"], status["nonfinite"], status["samples"]) == (int(finite.sum()), int((~finite).sum()), 1), status
    active, st = bake.render_adaptive(1, 0.0)
    assert active == int(finite.sum()) and st["points"] == active and st["paths"] == active, (active, st)
    rad2, cnt2 = big_reference(2)
    ni = bake.point_samples()
    assert np.array_equal(ni, np.where(finite, 2, 1))
    values2, queries2 = bake.values(queries=True)
    assert np.array_equal(bits(values2)[finite], bits(rad2)[finite]) and np.array_equal(queries2[finite], cnt2[finite].astype(np.uint64))
    assert np.array_equal(bits(values2)[~finite], bits(values1)[~finite]) and np.array_equal(queries2[~finite], queries1[~finite])
    assert st["rays"] == int((cnt2[finite].astype(np.uint64) - cnt1[finite]).sum())
    assert bake.status(0.0)["samples"] == 2
