"""The film at the sizes that take the paths the other film tests never reach (film.hip, film_abi.cpp, abi.cpp
enqueue_local), bit for bit against the CPU oracle like them:

(a) passes of 8 full chunks and more on a film that holds samples, 9 and more on an empty one: the unrolled body of
    film_accumulate_kernel, with every way into it (an assigned first chunk, a record read back, a tile list) and out of
    it (no tail, a tail of full chunks, a tail that ends in a short chunk);
(b) 1188 tiles: film_compact_kernel's scan across the sixteen waves of its workgroup and across two steps of 1024 tiles,
    the list of all tiles over a film whose tiles differ, and film passes cut into segments on the local-pool route;
(c) 3363 tiles: a share of more than 1024 tiles, four steps on the whole film, and a checkpoint whose records are more
    than the 8 MiB staging buffer.

The references come from tests/_film.py and the vectorised replay of tests/_film_adaptive.py, once per scene and frame;
the tests read them and leave them unchanged."""
import functools
import time

import numpy as np
import pytest

import _film
import _film_adaptive as A
import _guided as G
import rayrs_amd
from rayrs_amd import tiles

pytestmark = pytest.mark.gpu

SEED, BOUNCES, TAUS = _film.SEED, _film.BOUNCES, _film.TAUS
STEP = 1024           # tiles film_compact_kernel takes per step
SEGMENT = 65536       # the smallest rayrs_lab_tuning.local_segment_items


def same_bits(a, b):
    ui = np.uint64 if a.dtype == np.float64 else np.uint32
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(ui), np.ascontiguousarray(b).view(ui))


def differing(img, ref):
    return f"{int((img.view(np.uint64) != ref.view(np.uint64)).any(axis=-1).sum())} of {img.shape[0] * img.shape[1]} pixels differ"


class Setup:
    def __init__(self, name, local_pool, w, h):
        self.name, self.w, self.h = name, w, h
        self.desc = _film.DESCS[name](w, h)
        cam_args, objs, heur, env = self.desc
        self.scene = rayrs_amd.Scene(objs, 1e-6, 1e6, heur, env, device=0)
        self.scene.set_tuning(local_pool=local_pool)
        self.local = 1 if name == "sphere" and local_pool == 0 else 0
        assert self.scene.info()["local_pool"] == self.local
        self.cam = rayrs_amd.Camera(*cam_args)
        assert (self.cam.x_pixels(), self.cam.y_pixels()) == (w, h)

    def film(self, c, **kw):
        return rayrs_amd.Film(self.scene, self.cam, sample_chunk=c, max_bounces=BOUNCES, seed=SEED, **kw)


# ---- (a) long passes through the unrolled accumulate ----

LONG_W, LONG_H = 29, 19   # 4 x 3 tiles, padding on two edges
LONG_TAU = 0.5
# (chunk, passes): the full chunks of each pass against UNROLL = 8, as the module's docstring says.  A pass is a sample
# count, or ("adaptive", n, tau, cap): after one chunk every pixel is unconverged (M = 1), so that pass takes every tile,
# through the tile list, and the film stays uniform.
SEQUENCES = {
    "c1": (1, (9, 8, 17)),        # assigned chunk + one batch | exactly one batch, no tail | two batches and a tail of one
    "c2": (2, (34, 30, 19)),      # assigned chunk + two batches, no tail | one batch and a tail of 7 | one batch, a tail of one
                                  # full chunk and a short one: the film closes
    "c4": (4, (4, ("adaptive", 32, LONG_TAU, 36), 36)),   # one batch through the tile list | one batch and a tail of one
}
LONG_VARIANTS = [("sphere", 0), ("sphere", 1), ("mesh", 0)]
LONG_IDS = ["sphere-local-pool", "sphere-streaming", "mesh-streaming"]


@functools.lru_cache(maxsize=None)
def long_reference(name, seq):
    """Per pass of the sequence (N, the oracle's frame and stats at N, S1, S2, M from the traces)."""
    c, passes = SEQUENCES[seq]
    t0 = time.perf_counter()
    osc, ocam = _film.oracle_of(_film.DESCS[name](LONG_W, LONG_H))
    rgb = _film.named_traces(name, 83, LONG_W, LONG_H)   # (the longest sequence's samples, shared by all three)
    out, n = [], 0
    for p in passes:
        n += p if isinstance(p, int) else p[1]
        ref, ost = osc.render(ocam, n, BOUNCES, SEED, sample_chunk=c)
        frame, s1, s2, m = _film.expectation(rgb, c, n)
        assert same_bits(frame, ref), "the frame from the traces is not the oracle's"
        out.append((n, ref, ost, s1, s2, m))
    print(f"long_reference({name}, {seq}): {time.perf_counter() - t0:.2f} s of CPU-side reference")
    return out


def run_long_sequence(variant, seq, rank=0, ranks=1):
    s = Setup(*variant, LONG_W, LONG_H)
    c, passes = SEQUENCES[seq]
    film = s.film(c, tile_rank=rank, tile_ranks=ranks)
    mask = tiles.tile_mask(LONG_W, LONG_H, rank, ranks)
    share = (np.arange(12).reshape(3, 4) % ranks) == rank
    rays = paths = 0
    for p, (n, ref, ost, s1, s2, m) in zip(passes, long_reference(s.name, seq)):
        what = f"{variant} {seq} share {rank} of {ranks} after {n}"
        if isinstance(p, int):
            st = film.render(p)
        else:
            active, st = film.render_adaptive(*p[1:])
            assert active == int(share.sum()), what
        rays, paths = rays + st["rays"], paths + st["paths"]
        img = film.image(out_f64=True)
        assert (img[~mask] == 0).all() and not np.signbit(img[~mask]).any(), what
        assert np.array_equal(img[mask].view(np.uint64), ref[mask].view(np.uint64)), f"{what}: {differing(np.where(mask[..., None], img, ref), ref)}"
        assert np.array_equal(film.tile_samples(), np.where(share, n, 0)), what
        for tau in TAUS:
            fs = film.status(tau)
            assert (fs["unconverged"], fs["nonfinite"]) == _film.noise_counts(s1, s2, m, tau, mask), (what, tau)
            assert (fs["samples"], fs["full_chunks"], fs["closed"]) == (n, n // c, 1 if n % c else 0) and fs["full_chunks"] == m, what
            assert (fs["rays"], fs["paths"]) == (rays, paths), what
        if ranks == 1:
            assert (rays, paths) == (ost["rays"], ost["paths"]), what
        assert same_bits(film.noise(), G.noise_plane(s1, s2, np.where(share, n, 0), c, share)), what
    film.close()


@pytest.mark.parametrize("seq", sorted(SEQUENCES))
@pytest.mark.parametrize("variant", LONG_VARIANTS, ids=LONG_IDS)
def test_long_passes_add_their_chunks_in_order(variant, seq):
    run_long_sequence(variant, seq)


@pytest.mark.parametrize("variant", LONG_VARIANTS, ids=LONG_IDS)
def test_long_passes_on_a_tile_share(variant):
    run_long_sequence(variant, "c2", rank=1, ranks=3)


# ---- the replay's passes, and what they must look like to exercise the scan ----

def replay_passes(rep, passes, noise):
    """Runs ("uniform", n) and ("adaptive", n, tau, cap) on the replay: per pass its snapshot, with the counts at TAUS and
    at the pass's tau and, if asked for, the noise plane."""
    out = []
    for p in passes:
        snap = rep.uniform_pass(p[1]) if p[0] == "uniform" else rep.adaptive_pass(*p[1:])
        snap["counts"] = {tau: rep.counts(tau) for tau in TAUS + tuple(p[2:3])}
        snap["closed"], snap["c"], snap["share"] = rep.closed, rep.c, rep.share
        if noise:
            snap["noise"] = G.noise_plane(snap["s1"], snap["s2"], snap["nt"], rep.c, rep.share)
        out.append(snap)
    return out


def flags_per_step(snap):
    """The pass's flags in the order film_compact_kernel scans them -- the share's tiles, ascending -- cut into its steps."""
    flags = snap["active"].ravel()[snap["share"].ravel()]
    return [flags[at:at + STEP] for at in range(0, len(flags), STEP)]


def assert_the_scan_carries(snap, steps):
    """On the replay alone: the pass gives `before` something to carry across waves in the first step (more flagged tiles
    than one wave holds), `base` something to carry into every later step, and in every step a hole in front of a flagged
    tile, so that no list position is the tile's own index."""
    per_step = flags_per_step(snap)
    counts = [int(f.sum()) for f in per_step]
    assert len(per_step) == steps, (len(per_step), steps)
    assert 64 < counts[0] < len(per_step[0]), counts
    for f, k in zip(per_step[1:], counts[1:]):
        assert 1 <= k < len(f), counts
    for f in per_step:
        assert not f[:int(np.flatnonzero(f)[-1])].all(), "no unflagged tile precedes a flagged one"
    return counts


def run_pass(film, p):
    if p[0] == "uniform":
        return None, film.render(p[1])
    return film.render_adaptive(*p[1:])


def check_film(film, snap, what):
    """The film as it stands against the replay's snapshot: N_t, the frame, the counts, the noise plane if it is there."""
    share_px = np.repeat(np.repeat(snap["share"], 8, axis=0), 8, axis=1)[:snap["frame"].shape[0], :snap["frame"].shape[1]]
    nt = film.tile_samples()
    assert np.array_equal(nt, snap["nt"]) and not nt[~snap["share"]].any(), what
    img = film.image(out_f64=True)
    assert same_bits(img, snap["frame"]), f"{what}: {differing(img, snap['frame'])}"
    assert (img[~share_px] == 0).all() and not np.signbit(img[~share_px]).any(), what
    n_max = int(snap["nt"].max())
    for tau, want in snap["counts"].items():
        fs = film.status(tau)
        assert (fs["unconverged"], fs["nonfinite"]) == want, (what, tau)
        assert (fs["samples"], fs["full_chunks"], fs["closed"]) == (n_max, n_max // snap["c"], int(snap["closed"])), what
    if "noise" in snap:
        noise = film.noise()
        assert same_bits(noise, snap["noise"]), what
        assert (noise[~share_px] == 0).all() and not np.signbit(noise[~share_px]).any(), what


def check_pass(film, p, snap, what):
    active, st = run_pass(film, p)
    print(f"{what}: {snap['active_tiles']} tiles, rays {st['rays']} (replay {snap['rays']})")
    assert active is None or active == snap["active_tiles"], what
    assert (st["rays"], st["paths"]) == (snap["rays"], snap["paths"]), what
    check_film(film, snap, what)
    return st


# ---- (b) many tiles: the scan across waves and steps, segmented film passes ----

MANY_W, MANY_H, MANY_C = 288, 264, 4   # 36 x 33 = 1188 tiles: two steps
MANY_TILES = 36 * 33
MANY_TAU = {"sphere": 0.5, "mesh": 0.8}
MANY_SAMPLES = 28


def many_passes(tau):
    return (("uniform", 8), ("adaptive", 8, tau, 24), ("adaptive", 8, tau, 24), ("uniform", 4))


@functools.lru_cache(maxsize=None)
def many_reference(name):
    t0 = time.perf_counter()
    rgb, it = A.named_traces(name, MANY_SAMPLES, MANY_W, MANY_H)
    snaps = replay_passes(A.Replay(rgb, it, MANY_C), many_passes(MANY_TAU[name]), noise=True)
    first = replay_passes(A.Replay(rgb, it, 1), (("uniform", 8),), noise=False)[0]   # the c = 1 pass of the segmented variant
    print(f"many_reference({name}): {time.perf_counter() - t0:.2f} s of CPU-side reference; flagged per pass and step: "
          f"{[[int(f.sum()) for f in flags_per_step(s)] for s in snaps]}")
    return snaps, first


def launches(n_tiles, chunks_per_tile, segment=SEGMENT):
    """The local-pool route's launches for a pass (frame_plan.cpp plan_frame): segments of whole tiles, as many as hold `segment`
    items of 64 pixels x the pass's chunks per tile."""
    seg_tiles = -(-segment // (64 * chunks_per_tile))
    return -(-n_tiles // seg_tiles)


MANY_VARIANTS = [("sphere", 0, 0), ("sphere", 0, SEGMENT), ("sphere", 1, 0), ("mesh", 0, 0)]
MANY_IDS = ["sphere-local-pool", "sphere-local-pool-segmented", "sphere-streaming", "mesh-streaming"]


@pytest.mark.parametrize("variant", MANY_VARIANTS, ids=MANY_IDS)
def test_a_thousand_tiles_are_listed_across_waves_and_steps(variant):
    name, local_pool, segment = variant
    snaps, first_c1 = many_reference(name)
    passes = many_passes(MANY_TAU[name])
    # on the replay alone: the second adaptive pass makes the scan carry, the first step's tiles and the second's
    counts = assert_the_scan_carries(snaps[2], steps=2)
    assert snaps[0]["active_tiles"] == snaps[3]["active_tiles"] == MANY_TILES and len(np.unique(snaps[2]["nt"])) >= 2
    want = {"sphere": ([1188, 1186, 722, 1188], [615, 107]), "mesh": ([1188, 1177, 184, 1188], [94, 90])}[name]
    assert ([s["active_tiles"] for s in snaps], counts) == want
    s = Setup(name, local_pool, MANY_W, MANY_H)
    if name == "mesh":
        assert s.scene.info()["gate_n_wide"] > 1   # a real tree
    if segment:
        s.scene.lab_set(local_segment_items=segment)
        assert (launches(1188, 2), launches(722, 2), launches(1188, 1), launches(1188, 8)) == (3, 2, 2, 10)
    film = s.film(MANY_C)
    for k, (p, snap) in enumerate(zip(passes, snaps)):
        st = check_pass(film, p, snap, f"{variant} pass {k} {p}")
        assert st["local_pool"] == s.local
        if s.local:   # segments of whole tiles, or one launch: fails if segmentation silently stops happening
            assert st["kernel_launches"] == (launches(snap["active_tiles"], p[1] // MANY_C) if segment else 1), (k, st["kernel_launches"])
    film.close()
    if segment:   # one pass of 8 at c = 1: 8 chunks per tile, 128 tiles per segment, 10 segments, the last one short
        film = s.film(1)
        st = check_pass(film, ("uniform", 8), first_c1, f"{variant} c = 1")
        assert st["kernel_launches"] == 10
        film.close()


# ---- (c) a share of more than 1024 tiles, and a checkpoint in pieces ----

BIG_W, BIG_H, BIG_C, BIG_TAU = 472, 456, 4, 0.5   # 59 x 57 = 3363 tiles: four steps; share 2 of 3 has 1121: two
BIG_TILES = 59 * 57
BIG_PASSES = (("uniform", 8), ("adaptive", 8, BIG_TAU, 0), ("adaptive", 8, BIG_TAU, 0), ("uniform", 4))
STAGE_BYTES = 8 << 20   # film_abi.cpp's staging buffer


@functools.lru_cache(maxsize=None)
def big_reference(rank, ranks):
    t0 = time.perf_counter()
    rgb, it = A.named_traces("sphere", 28, BIG_W, BIG_H)   # (shared by the whole film and the share)
    snaps = replay_passes(A.Replay(rgb, it, BIG_C, rank=rank, ranks=ranks), BIG_PASSES, noise=False)
    print(f"big_reference({rank}, {ranks}): {time.perf_counter() - t0:.2f} s of CPU-side reference; flagged per pass and step: "
          f"{[[int(f.sum()) for f in flags_per_step(s)] for s in snaps]}")
    return snaps


@pytest.mark.parametrize("rank,ranks", [(0, 1), (2, 3)], ids=["whole-film", "share-2-of-3"])
def test_thousands_of_tiles_and_a_checkpoint_in_pieces(rank, ranks):
    snaps = big_reference(rank, ranks)
    n_local = tiles.local_tile_count(BIG_W, BIG_H, rank, ranks)
    assert n_local == (BIG_TILES if ranks == 1 else 1121) and int(snaps[0]["share"].sum()) == n_local
    # on the replay alone: the adaptive pass behind the checkpoint makes the scan carry in every step
    counts = assert_the_scan_carries(snaps[2], steps=4 if ranks == 1 else 2)
    flagged = [s["active_tiles"] for s in snaps[1:3]]
    assert (flagged, counts) == (([3361, 2029], [725, 425, 688, 191]) if ranks == 1 else ([1121, 683], [614, 69]))
    s = Setup("sphere", 0, BIG_W, BIG_H)
    film = s.film(BIG_C, tile_rank=rank, tile_ranks=ranks)
    for k in (0, 1):
        check_pass(film, BIG_PASSES[k], snaps[k], f"share {rank} of {ranks} pass {k}")
    image = film.state()
    records = BIG_TILES * 5 * 64 * 8
    assert records == 8609280 and STAGE_BYTES < records < 2 * STAGE_BYTES   # two pieces, the second one short
    assert len(image) == 88 + records + BIG_TILES * 4
    again = s.film(BIG_C, tile_rank=rank, tile_ranks=ranks)
    again.set_state(image)
    assert again.state() == image, "the image of the film the image was loaded into"
    check_film(again, snaps[1], "the loaded film")
    for k in (2, 3):
        for which, f in (("first film", film), ("loaded film", again)):
            check_pass(f, BIG_PASSES[k], snaps[k], f"share {rank} of {ranks} pass {k}, {which}")
        assert same_bits(film.image(out_f64=True), again.image(out_f64=True)) and np.array_equal(film.tile_samples(), again.tile_samples())
        assert film.status(BIG_TAU) == again.status(BIG_TAU)
    assert film.state() == again.state()
    film.close(), again.close()
