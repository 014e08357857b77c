"""What the noise-plane and guided-filter tests (test_guided.py, test_gpu_guided.py) expect (include/rayrs_hip.h NOISE PLANE
and GUIDED FILTER): the plane from S1, S2 and N_t with Python floats in the header's order, the filter as plain Python loops
in the header's order with exp taken from the oracle (_features.orc_exp).  Nothing here calls the library under test."""
import math

import numpy as np

import _features as F

INF = float("inf")
EPS = 2.0 ** -33
H3 = F.H3
G2 = (1.0 / 2.0, 1.0 / 4.0)


def noise_value(s1, s2, n_t, c):
    """One pixel of the share: Python floats are IEEE f64, nothing fused."""
    big_m = int(n_t) // int(c)
    m = float(big_m)
    if big_m < 2 or not math.isfinite(s1) or not math.isfinite(s2):
        return INF
    d = m * s2 - s1 * s1
    if not math.isfinite(d):
        return INF
    if not d > 0.0:
        return 0.0
    return d / (((m * m) * (m - 1.0)) * (float(c) * float(c)))


def noise_plane(s1, s2, tile_n, c, share=None):
    """(H, W) f64 from the S1 and S2 planes, N_t per 8x8 tile (tiles_y, tiles_x) and the chunk; share (tiles_y, tiles_x)
    bool, default every tile: pixels outside it read +0."""
    h, w = s1.shape
    a, b = s1.tolist(), s2.tolist()
    out = np.zeros((h, w))
    for y in range(h):
        for x in range(w):
            if share is not None and not share[y // 8, x // 8]:
                continue
            out[y, x] = noise_value(a[y][x], b[y][x], int(tile_n[y // 8, x // 8]), c)
    return out


def guided_level(color, var, normal, albedo, depth, step, kn, ka, kz, kv):
    """One level: (colour, variance).  An absent plane contributes no term: e is formed of the terms that are there."""
    h, w = color.shape[:2]
    c, v = color.tolist(), var.tolist()
    n = normal.tolist() if normal is not None else None
    a = albedo.tolist() if albedo is not None else None
    z = depth.tolist() if depth is not None else None
    oc = [[None] * w for _ in range(h)]
    ov = [[None] * w for _ in range(h)]
    for y in range(h):
        for x in range(w):
            cp = c[y][x]
            oc[y][x], ov[y][x] = cp, v[y][x]
            if not F._fin3(cp):
                continue
            gs = gw = 0.0
            for dy in range(-1, 2):
                qy = y + dy
                if qy < 0 or qy >= h:
                    continue
                for dx in range(-1, 2):
                    qx = x + dx
                    if qx < 0 or qx >= w:
                        continue
                    if not F._fin3(c[qy][qx]):
                        continue
                    vq = v[qy][qx]
                    if not vq >= 0.0:
                        continue
                    wt = G2[abs(dy)] * G2[abs(dx)]
                    gs += vq * wt
                    gw += wt
            r = 0.0 if gw == 0.0 else kv / (gs / gw + EPS)
            yp = (cp[0] + cp[1]) + cp[2]
            num, den, vs = [0.0, 0.0, 0.0], 0.0, 0.0
            for dy in range(-2, 3):
                qy = y + dy * step
                if qy < 0 or qy >= h:
                    continue
                for dx in range(-2, 3):
                    qx = x + dx * step
                    if qx < 0 or qx >= w:
                        continue
                    cq = c[qy][qx]
                    if not F._fin3(cq):
                        continue
                    vq = v[qy][qx]
                    if not vq >= 0.0:
                        continue
                    e = None  # ((dn*kn + da*ka) + dz*kz) + (dl*dl)*r_p over the terms that exist
                    if n is not None:
                        e = F._d2(n[y][x], n[qy][qx]) * kn
                    if a is not None:
                        term = F._d2(a[y][x], a[qy][qx]) * ka
                        e = term if e is None else e + term
                    if z is not None:
                        term = ((z[y][x] - z[qy][qx]) * (z[y][x] - z[qy][qx])) * kz
                        e = term if e is None else e + term
                    dl = yp - ((cq[0] + cq[1]) + cq[2])
                    term = (dl * dl) * r
                    e = term if e is None else e + term
                    if not math.isfinite(e):
                        continue
                    wgt = (H3[abs(dy)] * H3[abs(dx)]) * F.orc_exp(-e)
                    num[0] += cq[0] * wgt
                    num[1] += cq[1] * wgt
                    num[2] += cq[2] * wgt
                    den += wgt
                    ww = wgt * wgt
                    vs += 0.0 if ww == 0.0 else vq * ww
            if den == 0.0 or den * den == 0.0:
                continue
            oc[y][x] = [num[0] / den, num[1] / den, num[2] / den]
            ov[y][x] = vs / (den * den)
    return np.array(oc, dtype=np.float64).reshape(h, w, 3), np.array(ov, dtype=np.float64).reshape(h, w)


def guided_levels(color, var, normal, albedo, depth, levels, kn, ka, kz, kv):
    """Yields (colour, variance) after 1, 2, ... `levels` levels: level k has step 2^k."""
    cur = np.ascontiguousarray(color, dtype=np.float64)
    v = np.ascontiguousarray(var, dtype=np.float64)
    for k in range(levels):
        cur, v = guided_level(cur, v, normal, albedo, depth, 1 << k, kn, ka, kz, kv)
        yield cur, v


def guided(color, var, normal, albedo, depth, levels, kn, ka, kz, kv):
    out = None
    for out in guided_levels(color, var, normal, albedo, depth, levels, kn, ka, kz, kv):
        pass
    return out


def random_variance(seed, w, h):
    """A seeded variance plane with the awkward values in: 0, small values, +inf, one NaN and one negative."""
    rng = np.random.default_rng(seed)
    var = rng.uniform(0.0, 0.05, (h, w))
    n = w * h
    if n >= 8:
        flat = rng.permutation(n)
        k = max(1, n // 8)
        var.flat[flat[:k]] = 0.0
        var.flat[flat[k:2 * k]] = np.inf
        var.flat[flat[2 * k:3 * k]] = rng.uniform(1e-12, 1e-6, k)
        var.flat[flat[3 * k]] = np.nan
        var.flat[flat[3 * k + 1]] = -1.0
    return var
