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
    rgb, it = osc.path_trace_batch(ocam, n, seed, bounces, traversal=traversal)
    return rgb, it.astype(np.uint64)


@functools.lru_cache(maxsize=None)
def named_traces(name, n=CAP, w=W, h=H):
    osc, ocam = _film.oracle_of(_film.DESCS[name](w, h))
    return traces(osc, ocam, n)


class Replay:
    """A film as the header defines it, held as the per-tile sample counts N_t alone: everything else follows from the
    traces.  tile_rank / tile_ranks: the share, tiles t of the frame (row-major) with t % ranks == rank.

    Vectorised, so that frames of thousands of tiles replay in seconds: whatever is asked per tile is computed for the
    whole image once per distinct N_t (at) and then taken, or reduced, over the pixels whose tile holds that N_t.  This
    relies on two things.  A pixel's sums, frame value and predicate depend on its own samples and its tile's N_t alone,
    so the image evaluated at N is, on a tile with N_t = N, that tile evaluated alone -- bit for bit, the same numpy
    operations on the same operands.  And what is reduced over pixels or tiles are counts -- integers, whose sum has no
    order."""

    def __init__(self, rgb, iterations, c=C, rank=0, ranks=1):
        self.rgb, self.it, self.c = rgb, iterations, c
        self.h, self.w = rgb.shape[:2]
        self.ty, self.tx = (self.h + 7) // 8, (self.w + 7) // 8
        self.nt = np.zeros((self.ty, self.tx), dtype=np.uint32)
        index = np.arange(self.ty * self.tx).reshape(self.ty, self.tx)
        self.share = (index % ranks) == rank
        self.closed = False
        self._at = {}
        self._tile_counts = {}   # tau -> (unconverged[ty, tx], nonfinite[ty, tx]) for self.nt as it stands

    def at(self, n):
        """(frame, S1, S2, M) of the whole image after n samples per pixel; n = 0 is the empty film."""
        n = int(n)
        if n not in self._at:
            zero = np.zeros((self.h, self.w))
            self._at[n] = _film.expectation(self.rgb, self.c, n) if n else (np.zeros((self.h, self.w, 3)), zero, zero, 0)
        return self._at[n]

    def per_pixel(self, per_tile):
        """A per-tile array spread over the tiles' pixels in the image (clipped at its edge: padding is no pixel)."""
        return np.repeat(np.repeat(per_tile, 8, axis=0), 8, axis=1)[:self.h, :self.w]

    def per_tile(self, per_pixel):
        """The per-tile sums of a per-pixel array of counts."""
        padded = np.zeros((self.ty * 8, self.tx * 8), dtype=np.int64)
        padded[:self.h, :self.w] = per_pixel
        return padded.reshape(self.ty, 8, self.tx, 8).sum(axis=(1, 3))

    def tile_pixels(self, ty, tx):
        mask = np.zeros((self.h, self.w), dtype=bool)
        mask[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8] = True   # (clipped at the image's edge: padding is no pixel)
        return mask

    def tiles(self):
        return [(int(ty), int(tx)) for ty, tx in np.argwhere(self.share)]   # (row-major: ascending tile order)

    def levels(self):
        """(N, the share's pixels whose tile holds N samples) for every distinct N_t in the share."""
        nt_px, share_px = self.per_pixel(self.nt), self.per_pixel(self.share)
        return [(int(n), share_px & (nt_px == n)) for n in np.unique(self.nt[self.share])]

    def all_tile_counts(self, tau):
        """(unconverged[ty, tx], nonfinite[ty, tx]) among each tile's pixels, with the tile's own M; 0 outside the share."""
        if tau not in self._tile_counts:
            unc, nonf = np.zeros((self.h, self.w), dtype=bool), np.zeros((self.h, self.w), dtype=bool)
            for n, px in self.levels():
                _, s1, s2, m = self.at(n)
                u, f = _film.noise_masks(s1, s2, m, tau)
                unc[px], nonf[px] = u[px], f[px]
            self._tile_counts[tau] = self.per_tile(unc), self.per_tile(nonf)
        return self._tile_counts[tau]

    def tile_counts(self, ty, tx, tau):
        """(unconverged, nonfinite) among the tile's pixels, with the tile's own M."""
        unc, nonf = self.all_tile_counts(tau)
        return int(unc[ty, tx]), int(nonf[ty, tx])

    def counts(self, tau):
        unc, nonf = self.all_tile_counts(tau)
        return int(unc.sum()), int(nonf.sum())

    def frame(self):
        out = np.zeros((self.h, self.w, 3))
        for n, px in self.levels():
            out[px] = self.at(n)[0][px]
        return out

    def sums(self):
        """S1 and S2 per pixel, each tile at its own count."""
        s1, s2 = np.zeros((self.h, self.w)), np.zeros((self.h, self.w))
        for n, px in self.levels():
            s1[px], s2[px] = self.at(n)[1][px], self.at(n)[2][px]
        return s1, s2

    def select_mask(self, n, tau, cap=0):
        cap = min(cap, CURSOR_MAX) if cap else CURSOR_MAX
        return self.share & (self.nt.astype(np.int64) + n <= cap) & (self.all_tile_counts(tau)[0] > 0)

    def select(self, n, tau, cap=0):
        """The tiles a pass of n samples takes: room below the cap, and a pixel in the image that is unconverged at tau."""
        return [(int(ty), int(tx)) for ty, tx in np.argwhere(self.select_mask(n, tau, cap))]

    def _add(self, active, n):
        """n more samples for the tiles of the mask `active`: (rays, paths) of them."""
        rays = paths = 0
        nt_px, active_px = self.per_pixel(self.nt), self.per_pixel(active)
        for n0 in np.unique(self.nt[active]):
            n0 = int(n0)
            assert n0 + n <= self.it.shape[2], "the traces are shorter than the film"
            px = active_px & (nt_px == n0)
            rays += int(self.it[px][:, n0:n0 + n].sum())
            paths += int(px.sum()) * n
        self.nt[active] += np.uint32(n)
        self._tile_counts = {}
        return rays, paths

    def snapshot(self, active, rays, paths, tau):
        s1, s2 = self.sums()
        unc, nonf = self.counts(tau)
        return dict(active=active.copy(), active_tiles=int(active.sum()), nt=self.nt.copy(), frame=self.frame(), s1=s1, s2=s2,
                    unconverged=unc, nonfinite=nonf, rays=rays, paths=paths)

    def adaptive_pass(self, n, tau, cap=0):
        assert n > 0 and n % self.c == 0 and not self.closed
        active = self.select_mask(n, tau, cap)
        rays, paths = self._add(active, n)
        return self.snapshot(active, rays, paths, tau)

    def uniform_pass(self, n, tau=TAU):
        assert n > 0 and not self.closed
        active = self.share
        rays, paths = self._add(active, n)
        self.closed = n % self.c != 0
        return self.snapshot(active, rays, paths, tau)

    def pixel_samples(self):
        return int(self.per_pixel(self.nt)[self.per_pixel(self.share)].sum(dtype=np.int64))


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
