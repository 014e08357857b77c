"""A plain-Python reading of include/rayrs_hip.h AMBIENT OCCLUSION, independent of the library under test: the counter RNG
restated in Python integers (as tests/test_numeric.py does), the orthonormal basis written out (vecmath.rs:341-352), sin and
cos from the oracle's math functions, sqrt from numpy (correctly rounded, as IEEE asks), every operation an f64 numpy
operation on its own -- nothing fused -- in the header's order.  The verdict of a ray comes from the second reading of
geometry.rs and bvh.rs (tests/_geometry_reading.py) or from whatever closest-hit answers the caller hands to counts_from."""
import numpy as np

import _geometry_reading as G
import _oracle

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
PI = 3.14159265358979323846264338327950288


def mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def path_key(seed, pixel, sample):  # rr_path_key
    h = mix64((seed + GOLDEN) & M64)
    h = mix64(h ^ ((pixel * 0xD1B54A32D192ED03 + 0x8CB92BA72F3D8DD7) & M64))
    h = mix64(h ^ ((sample * 0xABC98388FB8FAC03 + 0x2545F4914F6CDD1D) & M64))
    return h


def uniform(key, draw):  # rr_uniform: 53 bits -> [0, 1)
    return float(mix64((key + (draw + 1) * GOLDEN) & M64) >> 11) * 2.0 ** -53


def onb(n):
    """vecmath.rs:341-352 on a vector of three arrays: e1 from the larger of |x|, |y|, e2 = (n x e1).unit()."""
    x, y, z = n
    zero = np.zeros_like(x)
    with np.errstate(all="ignore"):
        a = G.unit((z, zero, -x))
        b = G.unit((zero, z, -y))
        first = np.abs(x) > np.abs(y)
        e1 = tuple(np.where(first, a[k], b[k]) for k in range(3))
        e2 = G.unit(G.cross(n, e1))
    return e1, e2


def directions(normals, keys):
    """l of the header for every (normal, key) pair: (n, 3)."""
    n = G.vec(np.ascontiguousarray(normals, dtype=np.float64))
    u = np.array([uniform(int(k), 0) for k in keys])
    v = np.array([uniform(int(k), 1) for k in keys])
    e1, e2 = onb(n)
    phi = 2.0 * PI * v
    su = np.sqrt(u)
    sin, cos = _oracle.math_fn(0, phi), _oracle.math_fn(1, phi)
    with np.errstate(all="ignore"):
        l = G.add(G.add(G.scale(e1, cos * su), G.scale(e2, sin * su)), G.scale(n, np.sqrt(1.0 - u)))
    return np.stack(l, axis=1)


def rays(points, normals, samples, bias, seed, index_base=0, indices=None):
    """The n * samples rays of a call, point by point, sample by sample: (origins, directions), (n * samples, 3) each.
    indices: index_base + i of every point, where they are not consecutive (the image form's row * W + col)."""
    points, normals = (np.ascontiguousarray(a, dtype=np.float64) for a in (points, normals))
    n = len(points)
    indices = [int(index_base) + i for i in range(n)] if indices is None else [int(i) for i in indices]
    keys = [path_key(int(seed), i, s) for i in indices for s in range(samples)]
    rep_n = np.repeat(normals, samples, axis=0)
    with np.errstate(all="ignore"):
        o = np.stack(G.add(G.vec(np.repeat(points, samples, axis=0)), G.scale(G.vec(rep_n), float(bias))), axis=1)
    return o, directions(rep_n, keys)


def counts_from(t, obj, n, samples, t_max):
    """Per-point counts from the closest-hit answers of rays(): occ = a hit and t < t_max (None: anywhere)."""
    with np.errstate(all="ignore"):
        occ = (obj >= 0) if t_max is None else ((obj >= 0) & (t < t_max))
    return occ.reshape(n, samples).sum(axis=1).astype(np.uint32), occ


def visibility_from(counts, samples):
    return (np.int64(samples) - counts.astype(np.int64)).astype(np.float64) / np.float64(samples)


def turned(normals, d):
    """FEATURES' normal turned against the ray: n * -1.0 where n . d > 0.0."""
    normals = np.ascontiguousarray(normals, dtype=np.float64)
    with np.errstate(all="ignore"):
        flip = G.dot(G.vec(normals), G.vec(d)) > 0.0
    return np.where(flip[:, None], normals * -1.0, normals)
