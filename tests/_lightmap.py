"""The plain-Python reading of include/rayrs_hip.h LIGHTMAP ATLAS: coverage, owner, texel record, texel list and assembly, every
expression f64 in the header's order.  Two forms of each: a scalar one that follows the header line by line on Python floats, and
a vectorised numpy one of the same expressions, element by element, for atlases the scalar one would take minutes on
(tests/test_lightmap.py holds the two equal bit for bit on the small cases).  Nothing here calls the library."""
import math

import numpy as np

NO_OWNER = 0xFFFFFFFF
F = np.float64


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def same(a, b):
    """Bit for bit, a NaN being equal to any NaN (which NaN an operation gives is not specified)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def widen(verts):
    """f32 vertices widened exactly; f64 as they are."""
    return np.ascontiguousarray(verts).astype(np.float64)


def corner_uvs(uvs, idx):
    uvs = np.asarray(uvs, dtype=np.float64)
    return uvs if uvs.ndim == 3 else uvs[np.asarray(idx, dtype=np.int64)]


# ---- the triangles' normals (Triangle::new, geometry.rs:341-353), one form: numpy scalars element by element

def normals(verts, idx, flip=False):
    v, idx = widen(verts), np.asarray(idx, dtype=np.int64).reshape(-1, 3)
    p0, p1, p2 = v[idx[:, 0]], v[idx[:, 1]], v[idx[:, 2]]
    e1, e2 = p1 - p0, p2 - p0
    with np.errstate(all="ignore"):
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        mag = np.sqrt((nx * nx + ny * ny) + nz * nz)
        inv = 1.0 / mag
        n = np.stack([nx * inv, ny * inv, nz * inv], axis=-1)
    return -n if flip else n


# ---- the scalar form

def setup(uv, W, H):
    """COVERAGE's set-up of one triangle: (U0, V0, U1, V1, U2, V2, area2, negated), or None if it covers nothing."""
    (u0, v0), (u1, v1), (u2, v2) = [(float(a), float(b)) for a, b in uv]
    fw, fh = float(W), float(H)
    U0, V0, U1, V1, U2, V2 = u0 * fw, v0 * fh, u1 * fw, v1 * fh, u2 * fw, v2 * fh
    if not all(math.isfinite(t) for t in (U0, V0, U1, V1, U2, V2)):
        return None
    area2 = (U1 - U0) * (V2 - V0) - (V1 - V0) * (U2 - U0)
    negated = area2 < 0.0
    if negated:
        area2 = -area2
    if not math.isfinite(area2) or area2 == 0.0:
        return None
    return U0, V0, U1, V1, U2, V2, area2, negated


def edges(t, x, y):
    """(w0, w1, w2) at the centre of texel (x, y), negated with the triangle."""
    U0, V0, U1, V1, U2, V2, _, negated = t
    px, py = float(x) + 0.5, float(y) + 0.5
    w0 = (U2 - U1) * (py - V1) - (V2 - V1) * (px - U1)
    w1 = (U0 - U2) * (py - V2) - (V0 - V2) * (px - U2)
    w2 = (U1 - U0) * (py - V0) - (V1 - V0) * (px - U0)
    return (-w0, -w1, -w2) if negated else (w0, w1, w2)


def candidates(lo, hi, n):
    return [x for x in range(n) if float(x + 1) >= lo and float(x) <= hi]


def owner_scalar(uvs, W, H):
    """The owner plane, (H, W) uint32."""
    own = np.full((H, W), NO_OWNER, dtype=np.uint32)
    for k, uv in enumerate(np.asarray(uvs, dtype=np.float64)):
        t = setup(uv, W, H)
        if t is None:
            continue
        xs = candidates(min(t[0], t[2], t[4]), max(t[0], t[2], t[4]), W)
        ys = candidates(min(t[1], t[3], t[5]), max(t[1], t[3], t[5]), H)
        for y in ys:
            for x in xs:
                w0, w1, w2 = edges(t, x, y)
                if w0 >= 0.0 and w1 >= 0.0 and w2 >= 0.0 and k < own[y, x]:
                    own[y, x] = k
    return own


def atlas_scalar(verts, idx, uvs, W, H, flip=False):
    """(owner (H, W) uint32, index (n,) uint32, points, normals, bary (n, 3) f64)."""
    v, idx = widen(verts), np.asarray(idx, dtype=np.int64).reshape(-1, 3)
    uvs = corner_uvs(uvs, idx)
    own = owner_scalar(uvs, W, H)
    nrm = normals(v, idx, flip)
    index, points, nrms, bary = [], [], [], []
    for y in range(H):
        for x in range(W):
            k = int(own[y, x])
            if k == NO_OWNER:
                continue
            t = setup(uvs[k], W, H)
            _, w1, w2 = edges(t, x, y)
            b1, b2 = w1 / t[6], w2 / t[6]
            b0 = (1.0 - b1) - b2
            p0, p1, p2 = (v[idx[k, c]] for c in range(3))
            index.append(y * W + x)
            points.append([(b0 * float(p0[c]) + b1 * float(p1[c])) + b2 * float(p2[c]) for c in range(3)])
            nrms.append(nrm[k])
            bary.append((b0, b1, b2))
    shape = (len(index), 3)
    return (own, np.array(index, dtype=np.uint32), np.array(points, dtype=F).reshape(shape), np.array(nrms, dtype=F).reshape(shape),
            np.array(bary, dtype=F).reshape(shape))


def assemble_scalar(index, values, W, H, dilate):
    """(image (H, W, C), valid (H, W) bool)."""
    values = np.asarray(values, dtype=F)
    values = values.reshape(len(index), 1) if values.ndim == 1 else values
    C = values.shape[1]
    img, valid = np.zeros((H, W, C)), np.zeros((H, W), dtype=bool)
    for i, t in enumerate(index):
        img[int(t) // W, int(t) % W] = values[i]
        valid[int(t) // W, int(t) % W] = True
    with np.errstate(all="ignore"):
        for _ in range(dilate):
            new_img, new_valid, made = img.copy(), valid.copy(), False
            for y in range(H):
                for x in range(W):
                    if valid[y, x]:
                        continue
                    s, count = [F(0.0)] * C, 0
                    for dy in (-1, 0, 1):
                        for dx in (-1, 0, 1):
                            qx, qy = x + dx, y + dy
                            if 0 <= qx < W and 0 <= qy < H and valid[qy, qx]:
                                s = [s[c] + img[qy, qx, c] for c in range(C)]
                                count += 1
                    if count:
                        new_img[y, x] = [s[c] / F(count) for c in range(C)]
                        new_valid[y, x], made = True, True
            if not made:
                break
            img, valid = new_img, new_valid
    return img, valid


# ---- the vectorised form: the same expressions on arrays

def _setup_v(uvs, W, H):
    fw, fh = F(W), F(H)
    with np.errstate(all="ignore"):
        U, V = uvs[:, :, 0] * fw, uvs[:, :, 1] * fh
        area2 = (U[:, 1] - U[:, 0]) * (V[:, 2] - V[:, 0]) - (V[:, 1] - V[:, 0]) * (U[:, 2] - U[:, 0])
    negated = area2 < 0.0
    area2 = np.where(negated, -area2, area2)
    live = np.isfinite(U).all(axis=1) & np.isfinite(V).all(axis=1) & np.isfinite(area2) & (area2 != 0.0)
    return U, V, area2, negated, live


def _span_v(lo, hi, n):
    """first and count of the integers x of 0 .. n - 1 with x + 1 >= lo and x <= hi (lo, hi finite arrays)."""
    first = np.clip(np.ceil(np.clip(lo, 0.0, float(n) + 1.0)) - 1.0, 0.0, None)
    last = np.clip(np.floor(np.clip(hi, -1.0, float(n))), None, float(n - 1))
    count = np.where((hi >= 0.0) & (lo <= float(n)), np.maximum(last - first + 1.0, 0.0), 0.0)
    return first.astype(np.int64), count.astype(np.int64)


def _edges_v(U, V, negated, px, py):
    """w0, w1, w2 with the triangles' arrays broadcast against the centres'."""
    with np.errstate(all="ignore"):
        w0 = (U[2] - U[1]) * (py - V[1]) - (V[2] - V[1]) * (px - U[1])
        w1 = (U[0] - U[2]) * (py - V[2]) - (V[0] - V[2]) * (px - U[2])
        w2 = (U[1] - U[0]) * (py - V[0]) - (V[1] - V[0]) * (px - U[0])
    return tuple(np.where(negated, -w, w) for w in (w0, w1, w2))


def owner_vector(uvs, W, H, small=8):
    uvs = np.asarray(uvs, dtype=np.float64).reshape(-1, 3, 2)
    own = np.full(W * H, NO_OWNER, dtype=np.uint32)
    U, V, area2, negated, live = _setup_v(uvs, W, H)
    Uf, Vf = np.where(live[:, None], U, 0.0), np.where(live[:, None], V, 0.0)
    x0, bw = _span_v(Uf.min(axis=1), Uf.max(axis=1), W)
    y0, bh = _span_v(Vf.min(axis=1), Vf.max(axis=1), H)
    live = live & (bw > 0) & (bh > 0)
    # the small boxes, all at once over a small x small window; the others one triangle at a time over its own box
    batch = np.flatnonzero(live & (bw <= small) & (bh <= small))
    if len(batch):
        dx, dy = np.meshgrid(np.arange(small), np.arange(small))                      # (small, small)
        x, y = x0[batch, None, None] + dx, y0[batch, None, None] + dy
        inside = (dx < bw[batch, None, None]) & (dy < bh[batch, None, None])
        Ub, Vb = [U[batch, c, None, None] for c in range(3)], [V[batch, c, None, None] for c in range(3)]
        w0, w1, w2 = _edges_v(Ub, Vb, negated[batch, None, None], x.astype(F) + 0.5, y.astype(F) + 0.5)
        hit = inside & (w0 >= 0.0) & (w1 >= 0.0) & (w2 >= 0.0)
        k = np.broadcast_to(batch[:, None, None], hit.shape)
        np.minimum.at(own, (y * W + x)[hit], k[hit].astype(np.uint32))
    for k in np.flatnonzero(live & ~((bw <= small) & (bh <= small))):
        x, y = np.meshgrid(np.arange(x0[k], x0[k] + bw[k]), np.arange(y0[k], y0[k] + bh[k]))
        w0, w1, w2 = _edges_v(U[k], V[k], negated[k], x.astype(F) + 0.5, y.astype(F) + 0.5)
        hit = (w0 >= 0.0) & (w1 >= 0.0) & (w2 >= 0.0)
        at = (y * W + x)[hit]
        own[at] = np.minimum(own[at], np.uint32(k))
    return own.reshape(H, W)


def atlas_vector(verts, idx, uvs, W, H, flip=False, small=8):
    v, idx = widen(verts), np.asarray(idx, dtype=np.int64).reshape(-1, 3)
    uvs = corner_uvs(uvs, idx).reshape(-1, 3, 2)
    own = owner_vector(uvs, W, H, small)
    index = np.flatnonzero(own.reshape(-1) != NO_OWNER)
    k = own.reshape(-1)[index].astype(np.int64)
    U, V, area2, negated, _ = _setup_v(uvs[k], W, H)
    px, py = (index % W).astype(F) + 0.5, (index // W).astype(F) + 0.5
    _, w1, w2 = _edges_v([U[:, c] for c in range(3)], [V[:, c] for c in range(3)], negated, px, py)
    b1, b2 = w1 / area2, w2 / area2
    b0 = (1.0 - b1) - b2
    p0, p1, p2 = v[idx[k, 0]], v[idx[k, 1]], v[idx[k, 2]]
    points = (b0[:, None] * p0 + b1[:, None] * p1) + b2[:, None] * p2
    return own, index.astype(np.uint32), points.reshape(-1, 3), normals(v, idx, flip)[k].reshape(-1, 3), np.stack([b0, b1, b2], axis=-1).reshape(-1, 3)


def assemble_vector(index, values, W, H, dilate):
    values = np.asarray(values, dtype=F)
    values = values.reshape(len(index), 1) if values.ndim == 1 else values
    C = values.shape[1]
    img, valid = np.zeros((H * W, C)), np.zeros(H * W, dtype=bool)
    img[np.asarray(index, dtype=np.int64)] = values
    valid[np.asarray(index, dtype=np.int64)] = True
    img, valid = img.reshape(H, W, C), valid.reshape(H, W)
    with np.errstate(all="ignore"):
        for _ in range(dilate):
            pv = np.pad(valid, 1)
            pi = np.pad(img, ((1, 1), (1, 1), (0, 0)))
            s, count = np.zeros((H, W, C)), np.zeros((H, W), dtype=np.int64)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    nv = pv[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
                    ni = pi[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
                    s = np.where(nv[:, :, None], s + ni, s)
                    count = count + nv
            made = ~valid & (count > 0)
            if not made.any():
                break
            img = np.where(made[:, :, None], s / np.maximum(count, 1).astype(F)[:, :, None], img)
            valid = valid | made
    return img, valid


# ---- the small cases both test files go through: name -> (verts, idx, uvs (m, 3, 2), W, H, flip)

def _space(m, seed):
    """m triangles in space with their own three vertices each: (verts (3m, 3), idx (m, 3))."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-2.0, 2.0, size=(3 * m, 3)), np.arange(3 * m, dtype=np.uint32).reshape(m, 3)


def cases():
    from rayrs_amd import procedural, unwrap_triangles
    out = {}
    one_uv = np.array([[(0.1, 0.1), (0.9, 0.15), (0.3, 0.85)]])
    v1, i1 = _space(1, 1)
    out["one"] = (v1, i1, one_uv, 8, 8, False)
    out["flip"] = (v1, i1, one_uv, 8, 8, True)
    out["f32"] = (v1.astype(np.float32), i1, one_uv, 8, 8, False)
    quad_v = np.array([(0.0, 0.0, 0.0), (2.0, 0.0, 1.0), (2.0, 3.0, 1.0), (0.0, 3.0, 0.0)])
    quad_i = np.array([(0, 1, 2), (0, 2, 3)], dtype=np.uint32)
    corner = np.array([(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)])
    out["quad"] = (quad_v, quad_i, corner[quad_i.astype(np.int64)], 8, 8, False)          # the diagonal runs through texel centres
    rewound = np.array([(0, 1, 2), (0, 3, 2)], dtype=np.uint32)
    out["quad_rewound"] = (quad_v, rewound, corner[rewound.astype(np.int64)], 8, 8, False)
    v6, i6 = _space(6, 2)
    v6[9] = v6[10]                                                                        # triangle 3 has no area in space: a NaN normal
    bad = np.array([[(0.2, 0.2), (0.5, 0.5), (0.8, 0.8)],                                 # no area in the atlas
                    [(0.1, 0.6), (0.5, 0.7), (0.2, 0.95)],
                    [(np.nan, 0.1), (0.9, 0.1), (0.5, 0.9)],
                    [(0.55, 0.1), (0.95, 0.2), (0.6, 0.5)],
                    [(0.1, 0.1), (0.9, np.inf), (0.5, 0.9)],
                    [(0.05, 0.05), (0.45, 0.1), (0.1, 0.5)]])
    out["degenerate"] = (v6, i6, bad, 16, 16, False)
    v3, i3 = _space(3, 3)
    outside = np.array([[(-0.5, 0.2), (0.5, 0.1), (0.1, 0.9)], [(1.2, 0.2), (1.8, 0.3), (1.4, 0.9)], [(-1e6, -3.0), (-2.0, -1e300), (-5.0, -4.0)]])
    out["outside"] = (v3, i3, outside, 16, 12, False)
    out["full_67x35"] = (v1, i1, np.array([[(-0.1, -0.1), (2.5, -0.1), (-0.1, 2.5)]]), 67, 35, False)
    rng = np.random.default_rng(4)
    vt, it = _space(200, 5)
    at = rng.uniform(0.0, 1.0, size=(200, 1, 2))
    tiny = at + rng.uniform(-0.02, 0.02, size=(200, 3, 2))                                 # under 0.64 of a texel of a 16 x 16 atlas across
    out["tiny_200"] = (vt, it, tiny, 16, 16, False)
    v2, i2 = _space(2, 6)
    out["overlaid"] = (v2, i2, np.concatenate([one_uv, one_uv]), 8, 8, False)
    out["empty"] = (np.zeros((0, 3)), np.zeros((0, 3), dtype=np.uint32), np.zeros((0, 3, 2)), 5, 3, False)
    sv, si = procedural.icosphere(2)
    uv, w, h = unwrap_triangles(len(si), 8, 1)
    out["icosphere_320"] = (sv, si.astype(np.uint32), uv, w, h, False)
    return out
