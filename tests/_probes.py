"""A plain-Python reading of include/rayrs_hip.h SH PROBES, independent of the library under test: the keys and the draws come
from tests/_ao.py, a sample's direction is Sphere::sample on the unit sphere written out with the oracle's sin and cos and
numpy's sqrt (as tests/_lit.py light_sample), a path's value and its queries come from the readings that exist -- the oracle's
radiance() for the unlit paths, tests/_direct.py, _sky.py, _mesh.py and _tree.py for the lit ones, each started on the probe's ray
with the rng at draw 2 --, and the basis and the sums are written out in the header's order with one numpy f64 operation each."""
import numpy as np

import _ao
import _oracle
import _radiance

F = np.float64
PI = F(_ao.PI)
K0, K1, K2, K3, K4 = F(0.28209479177387814), F(0.4886025119029199), F(1.0925484305920792), F(0.31539156525252005), F(0.5462742152960396)
SKY = 0xFFFFFFFF


def direction(key):
    """w of the sample with this key: u1 = draw 0, u2 = draw 1."""
    u1, u2 = F(_ao.uniform(int(key), 0)), F(_ao.uniform(int(key), 1))
    with np.errstate(all="ignore"):
        phi = F(2.0) * PI * u2
        r = np.sqrt(u1 * (F(1.0) - u1))
        x = F(_oracle.math_fn(1, [phi])[0]) * F(2.0) * r
        y = F(_oracle.math_fn(0, [phi])[0]) * F(2.0) * r
        z = F(1.0) - F(2.0) * u1
    return x, y, z


def directions(n, samples, seed, index_base=0):
    """(n, S, 3): the w of every (i, s) of a call."""
    out = np.zeros((n, samples, 3))
    for i in range(n):
        for s in range(samples):
            out[i, s] = direction(_ao.path_key(int(seed), int(index_base) + i, s))
    out.setflags(write=False)
    return out


def basis(w):
    """Y_0 .. Y_8 on the components of w as they stand, every product from left to right."""
    x, y, z = (F(v) for v in w)
    with np.errstate(all="ignore"):
        return (K0, K1 * y, K1 * z, K1 * x, (K2 * x) * y, (K2 * y) * z, K3 * (((F(3.0) * z) * z) - F(1.0)), (K2 * x) * z,
                K4 * ((x * x) - (y * y)))


def project(values, w, sample_chunk):
    """coeffs (9, 3) of one probe from its samples' values (S, 3) and directions (S, 3): per chunk C[k][ch] from zero, += Y_k *
    L_s[ch] in sample order; the chunks added in chunk order, the first assigned; times FOUR_PI * (1.0 / S)."""
    samples = len(values)
    total = None
    with np.errstate(all="ignore"):
        for first, end in _radiance.chunks(samples, sample_chunk):
            c = [[F(0.0)] * 3 for _ in range(9)]
            for s in range(first, end):
                Y = basis(w[s])
                for k in range(9):
                    for ch in range(3):
                        term = Y[k] * F(values[s][ch])
                        c[k][ch] = c[k][ch] + term
            total = c if total is None else [[total[k][ch] + c[k][ch] for ch in range(3)] for k in range(9)]
        four_pi = F(4.0) * PI
        scale = four_pi * (F(1.0) / F(samples))
        return np.array([[total[k][ch] * scale for ch in range(3)] for k in range(9)])


def answers(values, queries, w, sample_chunk):
    """(coeffs (n, 9, 3) f64, queries (n,) uint32) of a call from its paths and its directions."""
    n = len(values)
    coeffs = np.stack([project(values[i], w[i], sample_chunk) for i in range(n)]) if n else np.zeros((0, 9, 3))
    return coeffs, np.asarray(queries).sum(axis=1).astype(np.uint32)


def _collect(points, samples, seed, index_base, one):
    n = len(points)
    values, queries = np.zeros((n, samples, 3)), np.zeros((n, samples), dtype=np.int64)
    w = np.zeros((n, samples, 3))
    for i in range(n):
        for s in range(samples):
            key = _ao.path_key(int(seed), int(index_base) + i, s)
            w[i, s] = direction(key)
            values[i, s], queries[i, s] = one(np.array(points[i], dtype=np.float64), w[i, s].copy(), key)
    for a in (values, queries, w):
        a.setflags(write=False)
    return values, queries, w


def unlit_paths(osc, points, samples, max_bounces, seed, index_base=0, traversal=0):
    """(values (n, S, 3), queries (n, S), directions (n, S, 3)) of an unlit call: the oracle's radiance() at draw 2."""
    return _collect(points, samples, seed, index_base,
                    lambda o, d, key: osc.radiance(o, d, max_bounces, key, 2, traversal)[:2])


def lit_paths(R, kind, points, samples, max_bounces, seed, lights, index_base=0):
    """The same of a call with lights, R a Reading of tests/_direct.py (kind "direct"), _sky.py ("sky": the sky is on),
    _mesh.py or _tree.py ("mesh", "tree": the group is the reading's); `lights` as the interface takes them, SKY among them."""
    lights = [int(k) for k in lights]
    lamps, sky = [k for k in lights if k != SKY], any(k == SKY for k in lights)
    assert kind in ("mesh", "tree") or sky == (kind == "sky")

    def one(o, d, key):
        if kind in ("mesh", "tree"):
            return R.path(o, d, max_bounces, key, 2, lamps, sky)[:2]
        return R.path(o, d, max_bounces, key, 2, lamps)[:2]
    return _collect(points, samples, seed, index_base, one)


def same_or_nan(got, want):
    """Bit-equal, or NaN on both sides (a NaN's payload is the hardware's business)."""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    return got.shape == want.shape and bool(((got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))).all())
