"""What the temporal-accumulation tests (test_temporal.py, test_gpu_temporal.py) expect: include/rayrs_hip.h TEMPORAL
ACCUMULATION read as plain Python -- Python floats (IEEE f64, nothing fused) and loops in the header's order -- with a tally
of the branch every pixel and every tap took; views built in closed form (analytic_view) with the awkward values written in;
and the case list the GPU comparison and the CPU tally check share.  Cameras come from the oracle.  Nothing here calls the
library under test."""
import functools
import math

import numpy as np

import _oracle

INF = float("inf")
MISS = 0xFFFFFFFF
PLANES = ("color", "variance", "weight", "normal", "albedo", "depth", "coverage", "object")
BRANCHES = ("pass_through", "empty", "no_source", "behind", "outside", "tap_outside", "tap_zero_b", "tap_nonfinite",
            "tap_bad_variance", "tap_zero_weight", "tap_object", "tap_depth", "tap_normal", "tap_not_background",
            "background_tap", "hit_tap", "no_valid_tap", "heal_frame", "heal_history", "cap_active", "blended")


class Cam:
    """A camera's fields as Python floats and ints, from a desc of the oracle's (or any struct with the same fields)."""

    def __init__(self, desc):
        self.origin, self.e_x, self.e_y, self.z = (tuple(float(c) for c in getattr(desc, k)) for k in ("origin", "e_x", "e_y", "z"))
        self.width, self.height = float(desc.width), float(desc.height)
        self.ppc, self.W, self.H = int(desc.ppc), int(desc.x_pixels), int(desc.y_pixels)


def oracle_cam(cam_args):
    return Cam(_oracle.OracleCamera(*cam_args).desc)


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def centre_ray(cam, r, col):
    """Step 2: the direction of the pixel's centre ray."""
    x = (float(cam.W - col) + 0.5) / float(cam.ppc) - cam.width / 2.
    y = (float(cam.H - r) + 0.5) / float(cam.ppc) - cam.height / 2.
    return tuple((cam.z[k] + x * cam.e_x[k]) + y * cam.e_y[k] for k in range(3))


def project(cam, u):
    """Step 4: (s, tp, fx, fy) of the vector u from cam's origin; tp, fx, fy are None unless s > 0."""
    s, zz = dot(u, cam.z), dot(cam.z, cam.z)
    if not s > 0.0:
        return s, None, None, None
    tp = s / zz
    xp, yp = (dot(u, cam.e_x) * zz) / s, (dot(u, cam.e_y) * zz) / s
    fx = (float(cam.W) + 0.5) - (xp + cam.width / 2.) * float(cam.ppc)
    fy = (float(cam.H) + 0.5) - (yp + cam.height / 2.) * float(cam.ppc)
    return s, tp, fx, fy


def _fin3(c):
    return math.isfinite(c[0]) and math.isfinite(c[1]) and math.isfinite(c[2])


def push(cam_a, a, cam_b, b, max_weight, depth_tol, normal_tol):
    """One push of view a (a dict of PLANES, "weight" being wc) into the history b (None: empty).  Returns (history, tally):
    the history after the push -- a's camera's planes with the three outputs -- and a dict counting BRANCHES."""
    tally = dict.fromkeys(BRANCHES, 0)
    tz2, tn2 = depth_tol * depth_tol, normal_tol * normal_tol
    H, W = cam_a.H, cam_a.W
    c, v, wc = a["color"].tolist(), a["variance"].tolist(), a["weight"].tolist()
    n, z, k, o = a["normal"].tolist(), a["depth"].tolist(), a["coverage"].tolist(), a["object"].tolist()
    if b is not None:
        bc, bv, bm = b["color"].tolist(), b["variance"].tolist(), b["weight"].tolist()
        bn, bz, bk, bo = b["normal"].tolist(), b["depth"].tolist(), b["coverage"].tolist(), b["object"].tolist()
    oc = [[None] * W for _ in range(H)]
    ov = [[None] * W for _ in range(H)]
    om = [[None] * W for _ in range(H)]
    for r in range(H):
        for col in range(W):
            cp, vp_in, w = c[r][col], v[r][col], wc[r][col]
            oc[r][col], ov[r][col], om[r][col] = cp, vp_in, w      # "no history"
            if not _fin3(cp) or not w > 0.0:                        # 1
                om[r][col] = w if w > 0.0 else 0.0
                tally["pass_through"] += 1
                continue
            if b is None:
                tally["empty"] += 1
                continue
            d = centre_ray(cam_a, r, col)                           # 2
            kp = k[r][col]                                          # 3
            hit = kp > 0.0
            if hit:
                big_t = z[r][col] / kp
                u = tuple((cam_a.origin[i] + d[i] * big_t) - cam_b.origin[i] for i in range(3))
            elif kp == 0.0:
                u = d
            else:
                tally["no_source"] += 1
                continue
            s, tp, fx, fy = project(cam_b, u)                       # 4
            if not s > 0.0:
                tally["behind"] += 1
                continue
            if not (fx >= -1.0 and fx < float(cam_b.W) and fy >= -1.0 and fy < float(cam_b.H)):
                tally["outside"] += 1
                continue
            x0f, y0f = math.floor(fx), math.floor(fy)
            ax, ay = fx - float(x0f), fy - float(y0f)
            x0, y0 = int(x0f), int(y0f)
            bs, hc, hv, hm = 0.0, [0.0, 0.0, 0.0], 0.0, 0.0         # 5
            for j in (0, 1):
                for i in (0, 1):
                    qy, qx = y0 + j, x0 + i
                    if qy < 0 or qy >= cam_b.H or qx < 0 or qx >= cam_b.W:
                        tally["tap_outside"] += 1
                        continue
                    bw = (ax if i else 1.0 - ax) * (ay if j else 1.0 - ay)
                    if bw == 0.0:
                        tally["tap_zero_b"] += 1
                        continue
                    cq = bc[qy][qx]
                    if not _fin3(cq):
                        tally["tap_nonfinite"] += 1
                        continue
                    vq, mq = bv[qy][qx], bm[qy][qx]
                    if not vq >= 0.0:
                        tally["tap_bad_variance"] += 1
                        continue
                    if not mq > 0.0:
                        tally["tap_zero_weight"] += 1
                        continue
                    kq = bk[qy][qx]
                    if hit:
                        if not (kq > 0.0 and bo[qy][qx] == o[r][col]):
                            tally["tap_object"] += 1
                            continue
                        dt = bz[qy][qx] / kq - tp
                        if not dt * dt <= tz2 * (tp * tp):
                            tally["tap_depth"] += 1
                            continue
                        np_, nq = n[r][col], bn[qy][qx]
                        e = [np_[0] - nq[0], np_[1] - nq[1], np_[2] - nq[2]]
                        if not (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2] <= tn2:
                            tally["tap_normal"] += 1
                            continue
                        tally["hit_tap"] += 1
                    else:
                        if not kq == 0.0:
                            tally["tap_not_background"] += 1
                            continue
                        tally["background_tap"] += 1
                    bs += bw
                    hc[0] += cq[0] * bw
                    hc[1] += cq[1] * bw
                    hc[2] += cq[2] * bw
                    hv += vq * bw
                    hm += mq * bw
            if bs == 0.0:                                           # 6
                tally["no_valid_tap"] += 1
                continue
            big_c = [hc[0] / bs, hc[1] / bs, hc[2] / bs]            # 7
            big_v, m0 = hv / bs, hm / bs
            m = m0 if m0 < max_weight else max_weight
            if not m0 < max_weight:
                tally["cap_active"] += 1
            vp = vp_in if vp_in >= 0.0 else INF                     # 8
            if vp == INF and big_v < INF:
                vp = (big_v * m0) / w
                tally["heal_frame"] += 1
            elif big_v == INF and vp < INF:
                big_v = (vp * w) / m0
                tally["heal_history"] += 1
            alpha = w / (w + m)                                     # 9
            beta = 1.0 - alpha
            oc[r][col] = [big_c[i] * beta + cp[i] * alpha for i in range(3)]
            bb, aa = beta * beta, alpha * alpha
            tb = 0.0 if bb == 0.0 else big_v * bb
            ta = 0.0 if aa == 0.0 else vp * aa
            ov[r][col] = tb + ta
            om[r][col] = m + w
            tally["blended"] += 1
    out = dict(a)                                                   # 10
    out["color"] = np.array(oc, dtype=np.float64).reshape(H, W, 3)
    out["variance"] = np.array(ov, dtype=np.float64).reshape(H, W)
    out["weight"] = np.array(om, dtype=np.float64).reshape(H, W)
    return out, tally


# ------------------------------------------------------------------------------------------------------ views

FLOOR = (-3.0, 3.0, -3.0, 3.0)       # y = 0: x range, z range
WALL = (-1.0, 1.0, 0.0, 2.0, -1.0)   # z = -1: x range, y range


def analytic_view(cam, seed):
    """Consistent planes for a floor rectangle (object 0) and an upright rectangle (object 1, creased) as the centre rays of `cam` see
    them, intersected in closed form (depth = the ray parameter t, coverage 1; a miss: all +0 and MISS), with seeded colour,
    variance and weight, and the awkward values written in: NaN and +-inf colours, NaN, negative and +inf variances, zero
    weights."""
    rng = np.random.default_rng(seed)
    H, W = cam.H, cam.W
    view = dict(color=rng.uniform(0.0, 2.0, (H, W, 3)), variance=rng.uniform(0.0, 0.05, (H, W)),
                weight=rng.integers(2, 9, (H, W)).astype(np.float64) * 4.0, normal=np.zeros((H, W, 3)),
                albedo=np.zeros((H, W, 3)), depth=np.zeros((H, W)), coverage=np.zeros((H, W)),
                object=np.full((H, W), MISS, dtype=np.uint32))
    o = cam.origin
    for r in range(H):
        for col in range(W):
            d = centre_ray(cam, r, col)
            best = None
            if d[1] != 0.0:
                t = (0.0 - o[1]) / d[1]
                x, zz = o[0] + d[0] * t, o[2] + d[2] * t
                if t > 0.0 and FLOOR[0] <= x <= FLOOR[1] and FLOOR[2] <= zz <= FLOOR[3]:
                    best = (t, 0, (0.0, 1.0, 0.0), (0.8, 0.8, 0.8))
            if d[2] != 0.0:
                t = (WALL[4] - o[2]) / d[2]
                x, y = o[0] + d[0] * t, o[1] + d[1] * t
                if t > 0.0 and WALL[0] <= x <= WALL[1] and WALL[2] <= y <= WALL[3] and (best is None or t < best[0]):
                    # (a crease at x = 0: one object, two normals further apart than any tolerance the tests use)
                    best = (t, 1, (0.0, 0.0, 1.0) if x < 0.0 else (0.6, 0.0, 0.8), (0.5, 0.1, 0.1))
            if best is not None:
                view["depth"][r, col], view["coverage"][r, col] = best[0], 1.0
                view["object"][r, col], view["normal"][r, col], view["albedo"][r, col] = best[1], best[2], best[3]
    npix = W * H
    if npix >= 16:
        flat = rng.permutation(npix)
        k = max(1, npix // 16)
        at = lambda lo, count=1: (flat[lo:lo + count] // W, flat[lo:lo + count] % W)  # noqa: E731
        view["color"][at(0) + (0,)] = np.nan
        view["color"][at(1) + (1,)] = np.inf
        view["color"][at(2) + (2,)] = -np.inf
        view["variance"][at(3)] = np.nan
        view["variance"][at(4)] = -1.0
        view["variance"][at(5, k)] = np.inf
        view["weight"][at(5 + k, k)] = 0.0
        view["coverage"][at(5 + 2 * k)] = np.nan      # a pixel with no source vector
    return view


# ------------------------------------------------------------------------------------------------------ the cases

UP = (0.0, 1.0, 0.0)
SIZES = [(1, 1), (7, 5), (65, 5), (33, 17), (64, 48)]      # A's, as (W, H)
MAX_WEIGHT, DEPTH_TOL, NORMAL_TOL = 40.0, 0.02, 0.25


def cam_args(origin, lookat, fov, w, h, ppi=100):
    ppc = round(ppi * 2.54)
    return (origin, UP, lookat, fov, w / float(ppc), h / float(ppc), ppi)


def pairs(w, h):
    """(name, A's camera, B's camera) for an A of w x h: B identical; translated, yawed, with another fov and ppi -- each of
    another size than A --; and facing away."""
    a = cam_args((0.3, 1.5, 5.0), (0.0, 0.6, 0.0), 50.0, w, h)
    bw, bh = w + 3, h + 2
    return [("identical", a, a),
            ("translated", a, cam_args((0.55, 1.6, 5.2), (0.25, 0.7, 0.2), 50.0, bw, bh)),
            ("yawed", a, cam_args((0.3, 1.5, 5.0), (0.45, 0.6, 0.0), 50.0, bw, bh)),
            ("fov and ppi", a, cam_args((0.3, 1.5, 5.0), (0.0, 0.6, 0.0), 64.0, 2 * w + 1, 2 * h + 1, ppi=150)),
            ("facing away", a, cam_args((0.3, 1.5, 5.0), (0.6, 2.4, 10.0), 50.0, bw, bh))]


@functools.lru_cache(maxsize=None)
def image_case(size, pair):
    """One case of the image-level comparison: view B pushed into an empty history, view A on top, then a third view from A's
    camera on top of that (the weights have grown: the cap; the history holds zero weights).  Returns a dict: the two
    cameras' arguments, the three (camera key, view) pushes, the history the reading gives after each, and the tallies
    summed."""
    name, args_a, args_b = pairs(*size)[pair]
    cam_a, cam_b = oracle_cam(args_a), oracle_cam(args_b)
    seed = 1000 * size[0] + 10 * size[1] + pair
    pushes = [("b", analytic_view(cam_b, seed)), ("a", analytic_view(cam_a, seed + 1)), ("a", analytic_view(cam_a, seed + 2))]
    cams = {"a": cam_a, "b": cam_b}
    states, total = [], dict.fromkeys(BRANCHES, 0)
    hist, hist_cam = None, None
    for key, view in pushes:
        hist, tally = push(cams[key], view, hist_cam, hist, MAX_WEIGHT, DEPTH_TOL, NORMAL_TOL)
        hist_cam = cams[key]
        states.append(hist)
        for b in BRANCHES:
            total[b] += tally[b]
    return dict(name=name, args={"a": args_a, "b": args_b}, pushes=pushes, states=states, tally=total)
