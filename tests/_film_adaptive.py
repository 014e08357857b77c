"""What the adaptive film's tests (test_film_adaptive.py, test_gpu_film_adaptive.py) expect, from the CPU oracle alone:
per-sample radiance and per-sample iteration counts (`rgb` and `n` of OracleScene.path_traces), _film.expectation for the
pixels of a tile at the tile's own sample count, the predicate of _film.noise_counts with the tile's own M, and the
selection rule of include/rayrs_hip.h (ADAPTIVE PASSES) replayed pass by pass.  Nothing here calls the library under
test."""
import functools

import numpy as np

import _film

W, H, C, SEED, BOUNCES = 64, 48, _film.C, _film.SEED, _film.BOUNCES
PASS, TAU, CAP = 8, 0.5, 64
CURSOR_MAX = (1 << 30) - 1


def traces(osc, ocam, n, seed=SEED, bounces=BOUNCES, traversal=0):
    """(rgb[row, col, s, 3], iterations[row, col, s]) of the samples s < n of every pixel, as orc_render runs them."""
    h, w = ocam.y_pixels(), ocam.x_pixels()
    pixels = [(r, c) for r in range(h) for c in range(w) for _ in range(n)]
    samples = [s for _ in range(h * w) for s in range(n)]
    tr = osc.path_traces(ocam, pixels, samples, seed, bounces, cap=4, traversal=traversal)
    return np.ascontiguousarray(tr["rgb"]).reshape(h, w, n, 3), tr["n"].astype(np.uint64).reshape(h, w, n)


@functools.lru_cache(maxsize=None)
def named_traces(name, n=CAP, w=W, h=H):
    osc, ocam = _film.oracle_of(_film.DESCS[name](w, h))
    return traces(osc, ocam, n)


class Replay:
    """A film as the header defines it, held as the per-tile sample counts N_t alone: everything else follows from the
    traces.  tile_rank / tile_ranks: the share, tiles t of the frame (row-major) with t % ranks == rank."""

    def __init__(self, rgb, iterations, c=C, rank=0, ranks=1):
        self.rgb, self.it, self.c = rgb, iterations, c
        self.h, self.w = rgb.shape[:2]
        self.ty, self.tx = (self.h + 7) // 8, (self.w + 7) // 8
        self.nt = np.zeros((self.ty, self.tx), dtype=np.uint32)
        index = np.arange(self.ty * self.tx).reshape(self.ty, self.tx)
        self.share = (index % ranks) == rank
        self.closed = False
        self._at = {}

    def at(self, n):
        """(frame, S1, S2, M) of the whole image after n samples per pixel; n = 0 is the empty film."""
        n = int(n)
        if n not in self._at:
            zero = np.zeros((self.h, self.w))
            self._at[n] = _film.expectation(self.rgb, self.c, n) if n else (np.zeros((self.h, self.w, 3)), zero, zero, 0)
        return self._at[n]

    def tile_pixels(self, ty, tx):
        mask = np.zeros((self.h, self.w), dtype=bool)
        mask[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8] = True   # (clipped at the image's edge: padding is no pixel)
        return mask

    def tiles(self):
        return [(ty, tx) for ty in range(self.ty) for tx in range(self.tx) if self.share[ty, tx]]

    def tile_counts(self, ty, tx, tau):
        """(unconverged, nonfinite) among the tile's pixels, with the tile's own M."""
        _, s1, s2, m = self.at(self.nt[ty, tx])
        return _film.noise_counts(s1, s2, m, tau, self.tile_pixels(ty, tx))

    def counts(self, tau):
        per_tile = [self.tile_counts(ty, tx, tau) for ty, tx in self.tiles()]
        return sum(u for u, _ in per_tile), sum(f for _, f in per_tile)

    def frame(self):
        out = np.zeros((self.h, self.w, 3))
        for ty, tx in self.tiles():
            m = self.tile_pixels(ty, tx)
            out[m] = self.at(self.nt[ty, tx])[0][m]
        return out

    def sums(self):
        """S1 and S2 per pixel, each tile at its own count."""
        s1, s2 = np.zeros((self.h, self.w)), np.zeros((self.h, self.w))
        for ty, tx in self.tiles():
            m = self.tile_pixels(ty, tx)
            s1[m], s2[m] = self.at(self.nt[ty, tx])[1][m], self.at(self.nt[ty, tx])[2][m]
        return s1, s2

    def select(self, n, tau, cap=0):
        """The tiles a pass of n samples takes: room below the cap, and a pixel in the image that is unconverged at tau."""
        cap = min(cap, CURSOR_MAX) if cap else CURSOR_MAX
        return [(ty, tx) for ty, tx in self.tiles()
                if int(self.nt[ty, tx]) + n <= cap and self.tile_counts(ty, tx, tau)[0] > 0]

    def _add(self, tiles, n):
        rays = paths = 0
        for ty, tx in tiles:
            n0 = int(self.nt[ty, tx])
            window = self.it[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8, n0:n0 + n]
            assert window.shape[2] == n, "the traces are shorter than the film"
            rays += int(window.sum())
            paths += int(window.size)
            self.nt[ty, tx] = n0 + n
        return rays, paths

    def snapshot(self, active, rays, paths, tau):
        s1, s2 = self.sums()
        unc, nonf = self.counts(tau)
        mask = np.zeros((self.ty, self.tx), dtype=bool)
        for ty, tx in active:
            mask[ty, tx] = True
        return dict(active=mask, active_tiles=len(active), nt=self.nt.copy(), frame=self.frame(), s1=s1, s2=s2,
                    unconverged=unc, nonfinite=nonf, rays=rays, paths=paths)

    def adaptive_pass(self, n, tau, cap=0):
        assert n > 0 and n % self.c == 0 and not self.closed
        active = self.select(n, tau, cap)
        rays, paths = self._add(active, n)
        return self.snapshot(active, rays, paths, tau)

    def uniform_pass(self, n, tau=TAU):
        assert n > 0 and not self.closed
        active = self.tiles()
        rays, paths = self._add(active, n)
        self.closed = n % self.c != 0
        return self.snapshot(active, rays, paths, tau)

    def pixel_samples(self):
        return sum(int(self.nt[ty, tx]) * int(self.tile_pixels(ty, tx).sum()) for ty, tx in self.tiles())


def replay_until(rep, tau=TAU, step=PASS, cap=CAP):
    """rayrs_amd.render_until(adaptive=True) on the replay: (passes, reason)."""
    passes = []
    while True:
        unc, _ = rep.counts(tau)
        if rep.nt[rep.share].max(initial=0) > 0 and unc == 0:
            return passes, "converged"
        if cap < step:
            return passes, "max_samples"
        p = rep.adaptive_pass(step, tau, cap)
        if p["active_tiles"] == 0:
            return passes, "max_samples"
        passes.append(p)
