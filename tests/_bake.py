"""What the bake's tests (test_bake.py, test_gpu_bake.py) expect, from the plain-Python readings alone: the per-sample values and
closest-hit query counts of 130 rays and 130 points per family -- _radiance.irradiance_paths / radiance_paths for the unlit bake,
_direct.* for the direct-lit one, _sky.* for the sky's --, made once per (family, strategy, kind, walk) and folded by
_film.expectation and _film.noise_masks, each point at its own sample count, and by a per-point replay of include/rayrs_hip.h
BAKE's SELECTION.  Nothing here calls the library under test.

The families are tests/_film_direct.py's: `room` under the studio map with its two lamps, and `mesh1_light` under the gradient map
with its lamp (it streams, has a hot group and a fast walk of its own).  The rays are a fixed fan of 40 x 24 from the family's camera
position into the scene, 130 of those that hit something, spread evenly over them; the points are their closest hits by the oracle, the normal of
a point the unit vector back along its ray, which faces the ray whatever was hit.  130 points are three waves, the last of two
lanes: the indices 0, 63, 64, 65 and 129 are a wave's first and last lanes and the last point."""
import functools

import numpy as np

import _direct
import _film
import _film_direct as FD
import _oracle
import _radiance
import _sky

N_POINTS = 130
SIZES = (1, 63, 64, 65, 130)
C = 2
N_MAX = 9          # the longest bake of the tests: passes 2 + 4 + 3
SEED, BOUNCES, BIAS = FD.SEED, FD.BOUNCES, 1e-4
STRATEGIES = ("unlit", "direct", "sky")
KINDS = ("irradiance", "radiance")
TAUS = _film.TAUS
CURSOR_MAX = (1 << 30) - 1


def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.sqrt((v * v).sum(axis=-1, keepdims=True))


@functools.lru_cache(maxsize=None)
def oracle(name):
    cam_args, objs, heur, hdri, lamps = FD.description(name)
    return _oracle.OracleScene(objs, FD.Z_NEAR, FD.Z_FAR, heur, hdri)


@functools.lru_cache(maxsize=None)
def geometry(name):
    """(origins, directions, points, normals), (130, 3) f64 each: 130 of the fan's rays that hit, and their hits."""
    cam_args = FD.description(name)[0]
    eye, up, lookat = (np.asarray(cam_args[k], dtype=np.float64) for k in (0, 1, 2))
    fwd = unit(lookat - eye)
    right = unit(np.cross(fwd, up))
    upv = np.cross(right, fwd)
    fan = [fwd + right * (0.9 * (i - 19.5) / 19.5) + upv * (0.6 * (j - 11.5) / 11.5) for j in range(24) for i in range(40)]
    d = unit(np.array(fan))
    o = np.tile(eye, (len(d), 1))
    t, obj = oracle(name).intersect_batch(o, d, FD.Z_NEAR, FD.Z_FAR, nthreads=1)
    hit = np.flatnonzero(obj >= 0)
    assert len(hit) >= N_POINTS, (name, len(hit))
    hit = hit[np.linspace(0, len(hit) - 1, N_POINTS).astype(np.int64)]   # (130 of them, spread evenly over the fan)
    o, d, t = o[hit], d[hit], t[hit]
    p = o + d * t[:, None]
    out = tuple(np.ascontiguousarray(x) for x in (o, d, p, -d))
    for x in out:
        x.setflags(write=False)
    return out


def inputs(name, kind):
    """(a, b) of a bake of the kind over the family's 130 rays or points."""
    o, d, p, nrm = geometry(name)
    return (p, nrm) if kind == "irradiance" else (o, d)


def lights(name, strategy):
    """What Bake (or the matching query) takes as lights= and direct= for the strategy."""
    import rayrs_amd
    lamps = list(FD.description(name)[4])
    if strategy == "unlit":
        return dict()
    return dict(lights=lamps + [rayrs_amd.SKY] if strategy == "sky" else lamps, direct=True)


@functools.lru_cache(maxsize=None)
def paths(name, strategy, kind, fast=False):
    """(values (130, N_MAX, 3) f64, queries (130, N_MAX) uint64): sample s of point i with index_base = 0, from the reading of the
    strategy.  fast: the product's fast walk, registered by the GPU tests (FD.register_fast_walk)."""
    cam_args, objs, heur, hdri, lamps = FD.description(name)
    a, b = inputs(name, kind)
    if strategy == "unlit":
        osc, traversal = (FD._fast_oracles[name], 2) if fast else (oracle(name), 0)
        if kind == "irradiance":
            values, queries = _radiance.irradiance_paths(osc, a, b, N_MAX, BIAS, BOUNCES, SEED, traversal=traversal)
        else:
            values, queries = _radiance.radiance_paths(osc, a, b, N_MAX, BOUNCES, SEED, traversal=traversal)
    else:
        module = _sky if strategy == "sky" else _direct
        R = (module.Reading(objs, FD.Z_NEAR, FD.Z_FAR, heur, hdri, osc=FD._fast_oracles[name], traversal=2) if fast
             else module.Reading(objs, FD.Z_NEAR, FD.Z_FAR, heur, hdri))
        if kind == "irradiance":
            values, queries = module.irradiance_paths(R, a, b, N_MAX, BIAS, BOUNCES, SEED, lamps)
        else:
            values, queries = module.radiance_paths(R, a, b, N_MAX, BOUNCES, SEED, lamps)
    values, queries = np.array(values, dtype=np.float64), np.array(queries).astype(np.uint64)
    values.setflags(write=False), queries.setflags(write=False)
    return values, queries


def noise_plane(s1, s2, m, c):
    """include/rayrs_hip.h NOISE PLANE per point: s1, s2 (n,), m (n,) integers."""
    out = np.full(len(s1), np.inf)
    mf, cf = m.astype(np.float64), float(c)
    with np.errstate(all="ignore"):
        d = mf * s2 - s1 * s1
        v = d / (((mf * mf) * (mf - 1.0)) * (cf * cf))
    ok = (m >= 2) & np.isfinite(s1) & np.isfinite(s2) & np.isfinite(d)
    out[ok] = np.where(d[ok] > 0.0, v[ok], 0.0)
    return out


class Replay:
    """A bake as the header defines it, held as the per-point sample counts N_i alone: everything else follows from the paths.
    Whatever is asked per point is computed for all points once per distinct N (at), by _film.expectation on the points as a
    one-row image, and taken at the points that hold N: a point's sums and predicate depend on its own samples and N_i alone."""

    def __init__(self, values, queries, c=C, n_points=None):
        n_points = len(values) if n_points is None else n_points
        self.rgb = values[None, :n_points]          # (1, n, S, 3): _film.expectation's image
        self.q = queries[:n_points]
        self.c, self.n = c, n_points
        self.ni = np.zeros(n_points, dtype=np.uint32)
        self.closed = False
        self.rays = self.paths = 0
        self._at = {}

    def at(self, n):
        """(value (n, 3), S1, S2, M) of every point after n samples; n = 0 is the empty bake."""
        n = int(n)
        if n not in self._at:
            if n == 0:
                self._at[n] = (np.zeros((self.n, 3)), np.zeros(self.n), np.zeros(self.n), 0)
            else:
                frame, s1, s2, m = _film.expectation(self.rgb, self.c, n)
                self._at[n] = (frame[0], s1[0], s2[0], m)
        return self._at[n]

    def levels(self):
        return [(int(n), self.ni == n) for n in np.unique(self.ni)]

    def values(self):
        out = np.zeros((self.n, 3))
        for n, at in self.levels():
            out[at] = self.at(n)[0][at]
        return out

    def queries(self):
        return np.array([int(self.q[i, :self.ni[i]].sum()) for i in range(self.n)], dtype=np.uint64)

    def sums(self):
        s1, s2 = np.zeros(self.n), np.zeros(self.n)
        for n, at in self.levels():
            s1[at], s2[at] = self.at(n)[1][at], self.at(n)[2][at]
        return s1, s2

    def masks(self, tau):
        """(unconverged, nonfinite) per point, each with its own M_i."""
        unc, nonf = np.zeros(self.n, dtype=bool), np.zeros(self.n, dtype=bool)
        for n, at in self.levels():
            _, s1, s2, m = self.at(n)
            u, f = _film.noise_masks(s1, s2, m, tau)
            unc[at], nonf[at] = u[at], f[at]
        return unc, nonf

    def counts(self, tau):
        unc, nonf = self.masks(tau)
        return int(unc.sum()), int(nonf.sum())

    def noise(self):
        s1, s2 = self.sums()
        return noise_plane(s1, s2, self.ni // self.c, self.c)

    def select(self, n, tau, cap=0):
        """SELECTION: room for n more samples below the cap, and unconverged at tau."""
        cap = min(cap, CURSOR_MAX) if cap else CURSOR_MAX
        return (self.ni.astype(np.int64) + n <= cap) & self.masks(tau)[0]

    def _add(self, active, n):
        rays = sum(int(self.q[i, self.ni[i]:self.ni[i] + n].sum()) for i in np.flatnonzero(active))
        assert int(self.ni[active].max(initial=0)) + n <= self.q.shape[1], "the paths are shorter than the bake"
        paths = int(active.sum()) * n
        self.ni[active] += np.uint32(n)
        self.rays, self.paths = self.rays + rays, self.paths + paths
        return dict(active=active.copy(), points=int(active.sum()), rays=rays, paths=paths, ni=self.ni.copy(), values=self.values(),
                    queries=self.queries())

    def adaptive_pass(self, n, tau, cap=0):
        assert n > 0 and n % self.c == 0 and not self.closed
        return self._add(self.select(n, tau, cap), n)

    def uniform_pass(self, n):
        assert n > 0 and not self.closed
        out = self._add(np.ones(self.n, dtype=bool), n)
        self.closed = n % self.c != 0
        return out
