"""What the feature-buffer and denoiser tests (test_features.py, test_gpu_features.py, test_gpu_denoise.py) expect,
computed from the CPU oracle alone (include/rayrs_hip.h FEATURES and DENOISER): the first hit of every (pixel, sample) from
OracleScene.path_traces(max_bounces=1, cap=1), the primary ray from OracleCamera.primary_ray with the path key, position and
normal from the second reading of geometry.rs (_geometry_reading.py), albedo from the scene description, sums sequential in
f64; the a-trous filter as plain Python loops in the header's order with exp taken from the oracle.  Nothing here calls the
library under test."""
import functools
import math

import numpy as np

import _film
import _geometry_reading as G
import _oracle
from rayrs_amd import tiles
from rayrs_amd.api import MAT_NO_REFLECT, flatten_objects
from test_numeric import path_key

MISS = 0xFFFFFFFF
PLANES = ("normal", "albedo", "depth", "coverage", "object")


def object_table(objs):
    """One entry per object in insertion order (a mesh is one object per triangle, lib.rs:407): (normal_of(position),
    albedo)."""
    table = []
    for o in flatten_objects(objs):
        albedo = (0.0, 0.0, 0.0) if o.mat.kind == MAT_NO_REFLECT else tuple(float(c) for c in o.mat.color)
        if o.kind == "sphere":
            c = tuple(float(x) for x in o.origin)
            table.append((lambda p, c=c: G.sphere_normal(c, p), albedo))
        elif o.kind == "plane":
            n = G.plane_normal(o.axis)
            table.append((lambda p, n=n: n, albedo))
        elif o.kind == "triangle":
            n = G.triangle_new(*[tuple(float(x) for x in p) for p in o.p])[2]
            table.append((lambda p, n=n: n, albedo))
        elif o.kind == "mesh":
            v = np.asarray(o.verts, dtype=np.float64)  # f32 -> f64 is exact
            for i, j, k in np.asarray(o.idx):
                n = G.triangle_new(tuple(v[i]), tuple(v[j]), tuple(v[k]))[2]
                table.append((lambda p, n=n: n, albedo))
        else:
            raise ValueError(o.kind)
    return table


def sample_features(desc, samples, seed=_film.SEED):
    """Per-sample values: dict of normal[h, w, F, 3], albedo[h, w, F, 3], depth[h, w, F], coverage[h, w, F], obj[h, w, F]
    (int64, -1 = miss)."""
    cam_args, objs, heur, env = desc
    osc, ocam = _film.oracle_of(desc)
    table = object_table(objs)
    h, w = ocam.y_pixels(), ocam.x_pixels()
    pixels = [(r, c) for r in range(h) for c in range(w) for _ in range(samples)]
    sidx = [s for _ in range(h * w) for s in range(samples)]
    tr = osc.path_traces(ocam, pixels, sidx, seed, max_bounces=1, cap=1)
    assert (tr["n"] == 1).all()
    obj = tr["obj"][:, 0].reshape(h, w, samples)
    t = tr["t"][:, 0].reshape(h, w, samples)
    out = dict(normal=np.zeros((h, w, samples, 3)), albedo=np.zeros((h, w, samples, 3)), depth=np.zeros((h, w, samples)),
               coverage=np.zeros((h, w, samples)), obj=obj)
    for r in range(h):
        for c in range(w):
            for s in range(samples):
                k = int(obj[r, c, s])
                if k < 0:
                    continue  # a miss: all four are +0
                key = path_key(seed, r * w + c, s)
                o, d, _ = ocam.primary_ray(h - r, w - c, key)  # the render's flipped indices (main.rs:74-75)
                tt = float(t[r, c, s])
                position = G.point(tuple(float(x) for x in o), tuple(float(x) for x in d), tt)
                normal_of, albedo = table[k]
                out["normal"][r, c, s] = normal_of(position)
                out["albedo"][r, c, s] = albedo
                out["depth"][r, c, s] = tt
                out["coverage"][r, c, s] = 1.0
    return out


def sequential_mean(v, n):
    """sum over s = 0 .. n-1 in sample order, the first value assigned, then * (1.0 / n)."""
    total = v[:, :, 0].copy()
    for s in range(1, n):
        total = total + v[:, :, s]
    return total * (1.0 / float(n))


def features_from(per_sample, n, rank=0, ranks=1):
    """The five planes for the first n samples and a tile share; pixels outside the share read +0 and 0xFFFFFFFF."""
    h, w = per_sample["depth"].shape[:2]
    mask = tiles.tile_mask(w, h, rank, ranks)
    out = {k: sequential_mean(per_sample[k], n) for k in ("normal", "albedo", "depth", "coverage")}
    first = per_sample["obj"][:, :, 0]
    out["object"] = np.where(first < 0, MISS, first).astype(np.uint32)
    for k in ("normal", "albedo", "depth", "coverage"):
        out[k] = np.where(mask[..., None] if out[k].ndim == 3 else mask, out[k], 0.0)
    out["object"] = np.where(mask, out["object"], np.uint32(MISS)).astype(np.uint32)
    return out


@functools.lru_cache(maxsize=None)
def named_samples(name, samples, w=_film.W, h=_film.H):
    return sample_features(_film.DESCS[name](w, h), samples)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    view = {8: np.uint64, 4: np.uint32}[a.dtype.itemsize]
    return bool(np.array_equal(a.view(view), b.view(view)))


# ------------------------------------------------------------------------------------------------------ the filter

H3 = (3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)


def orc_exp(x):
    return float(_oracle.lib().orc_math(4, float(x), 0.0))


def _fin3(c):
    return math.isfinite(c[0]) and math.isfinite(c[1]) and math.isfinite(c[2])


def _d2(a, b):
    dx, dy, dz = a[0] - b[0], a[1] - b[1], a[2] - b[2]
    return (dx * dx + dy * dy) + dz * dz


def atrous_level(color, normal, albedo, depth, step, kn, ka, kz, kc_k):
    """One level, include/rayrs_hip.h DENOISER: Python floats (IEEE f64, nothing fused), loops in the header's order.  An
    absent plane contributes no term: the sum e is formed of the terms that are there, in the header's order."""
    h, w = color.shape[:2]
    c = color.tolist()
    n = normal.tolist() if normal is not None else None
    a = albedo.tolist() if albedo is not None else None
    z = depth.tolist() if depth is not None else None
    out = [[None] * w for _ in range(h)]
    for y in range(h):
        for x in range(w):
            cp = c[y][x]
            if not _fin3(cp):
                out[y][x] = cp
                continue
            num, den = [0.0, 0.0, 0.0], 0.0
            for dy in range(-2, 3):
                qy = y + dy * step
                if qy < 0 or qy >= h:
                    continue
                for dx in range(-2, 3):
                    qx = x + dx * step
                    if qx < 0 or qx >= w:
                        continue
                    cq = c[qy][qx]
                    if not _fin3(cq):
                        continue
                    e = None  # ((dn*kn + da*ka) + dz*kz) + dc*kc_k over the terms that exist
                    if n is not None:
                        e = _d2(n[y][x], n[qy][qx]) * kn
                    if a is not None:
                        term = _d2(a[y][x], a[qy][qx]) * ka
                        e = term if e is None else e + term
                    if z is not None:
                        dzz = (z[y][x] - z[qy][qx]) * (z[y][x] - z[qy][qx])
                        term = dzz * kz
                        e = term if e is None else e + term
                    term = _d2(cp, cq) * kc_k
                    e = term if e is None else e + term
                    if not math.isfinite(e):
                        continue
                    wgt = (H3[abs(dy)] * H3[abs(dx)]) * orc_exp(-e)
                    num[0] += cq[0] * wgt
                    num[1] += cq[1] * wgt
                    num[2] += cq[2] * wgt
                    den += wgt
            out[y][x] = cp if den == 0.0 else [num[0] / den, num[1] / den, num[2] / den]
    return np.array(out, dtype=np.float64).reshape(h, w, 3)


def atrous_levels(color, normal, albedo, depth, levels, kn, ka, kz, kc):
    """Yields the frame after 1, 2, ... `levels` levels: level k has step 2^k and kc_k = kc * 4^k."""
    cur = np.ascontiguousarray(color, dtype=np.float64)
    for k in range(levels):
        cur = atrous_level(cur, normal, albedo, depth, 1 << k, kn, ka, kz, kc * (4.0 ** k))
        yield cur


def atrous(color, normal, albedo, depth, levels, kn, ka, kz, kc):
    out = None
    for out in atrous_levels(color, normal, albedo, depth, levels, kn, ka, kz, kc):
        pass
    return out


def k_of(sigma):
    """rayrs_amd.api._k restated: 1 / sigma^2, None or inf -> 0."""
    if sigma is None or sigma == float("inf"):
        return 0.0
    return 1.0 / (float(sigma) * float(sigma))


def random_case(seed, w, h):
    """Seeded inputs with the awkward values in: colour pixels that are NaN, +inf and -inf, NaN normals."""
    rng = np.random.default_rng(seed)
    color = rng.uniform(0.0, 2.0, (h, w, 3))
    normal = rng.normal(size=(h, w, 3))
    normal /= np.linalg.norm(normal, axis=2, keepdims=True)
    albedo = rng.choice([0.1, 0.5, 0.8], size=(h, w, 1)) * np.ones((1, 1, 3))
    depth = rng.uniform(1.0, 20.0, (h, w))
    n = w * h
    if n >= 8:
        flat = rng.permutation(n)[:6]
        ys, xs = flat // w, flat % w
        color[ys[0], xs[0], 0] = np.nan
        color[ys[1], xs[1], 1] = np.inf
        color[ys[2], xs[2], 2] = -np.inf
        color[ys[3], xs[3]] = np.nan
        normal[ys[4], xs[4], 1] = np.nan
        normal[ys[5], xs[5]] = np.nan
    return color, normal, albedo, depth
