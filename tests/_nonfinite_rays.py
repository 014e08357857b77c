"""Rays with NaN, infinite, zero and far-scaled components for the ray queries (include/rayrs_hip.h RAY QUERIES: "any f64 is a
legal component"), and the conditions under which they test what they are made for.  tests/test_nonfinite_rays.py compares the
second reading (tests/_geometry_reading.py) with the oracle on them, tests/test_gpu_nonfinite_rays.py the kernels with both.

The classes are NOT families of _geometry_reading.FAMILIES: G.scene_rays concatenates a scene's cases and other tests select
from that concatenation by stride, so a new case there would move their inputs.

Every class is made from G.rays_for(scene, "general") base rays with a fixed seed:

  * corrupting classes put NaN, +-inf, +-0 or 5e-324 into components of a general ray;
  * scaling classes aim the base ray's origin at a point of a triangle or rectangle (of any primitive where the scene has
    neither) and multiply the direction by 2^k: t is then 2^-k times an ordinary one and leaves the window (1e-6, 1e6), den and
    the numerators of Triangle::intersect pass the 2^-500 and 2^500 of the hot group's shortcut, and a sphere's dot(d, d)
    overflows or underflows;
  * o_far_axis_k: o = (x, y + 2^k, z), d = (0, -2^k, 0) above a point (x, y, z) of a rectangle that faces y (of any primitive
    where the scene has none).  Adding 2^160 absorbs every coordinate of the scene, so both slabs of the root box give the
    same t and AxisAlignedBoundingBox::intersect's `tmax <= tmin` refuses the ray: these classes never enter the root box;
  * d_axis_k: the same direction from (x, y + h, z) with h in [1, 8): the axis-parallel far-scaled ray that does hit.

Each class lies in the batch twice, because the hot group's shortcut returns early only when every live lane of a wave is
settled and the walks' wave votes depend on the neighbours: as a run of RUN = 256 consecutive rays that begins at a multiple
of 256 (whole waves and workgroups of one class), and ray by ray between ordinary general rays.  A tail of ordinary rays
makes the batch no multiple of 256."""
import numpy as np

import _geometry_reading as G
from test_hot_group import settled

RUN = 256
TAIL = 77
INF, NAN = float("inf"), float("nan")
WINDOWS = {"t0_t1": (G.T0, G.T1), "open": (0.0, INF), "wide": (2.0 ** -1060, 2.0 ** 1020)}
OPEN = ("open", "wide")
SCENES = ("mesh1280_light", "floor_spheres", "soup", "near_far_above_t0")
HOT_SCENES = ("mesh1280_light", "floor_spheres")
BUILDERS = [(s, "sah1000") for s in SCENES] + [("soup", "midpoint")]
SCALES = (400, 499, 500, 501, 600, 1000, -400, -499, -500, -501, -600, -1000)
FAR = (160, 520, 1000)

CORRUPT = ("d_nan_all", "d_nan_one", "o_nan_one", "o_nan_all", "d_pinf_one", "d_ninf_one", "o_pinf_one", "o_ninf_one",
           "o_pinf_d_pinf", "o_pinf_d_ninf", "d_pzero_inside", "d_nzero_inside", "d_denormal_one")
SCALED = tuple(f"scale_2^{k}" for k in SCALES)
FAR_AXIS = tuple(f"o_far_axis_{k}" for k in FAR)
D_AXIS = tuple(f"d_axis_{k}" for k in FAR)
CLASSES = CORRUPT + SCALED + FAR_AXIS + D_AXIS


def _flat_targets(prims, r, n, facing_y=False):
    """Points on triangles and rectangles (facing_y: on rectangles that face y), on any primitive where there is none."""
    kinds = (prims.kind == 1) & ((prims.axis >> 1) == 1) if facing_y else prims.kind != 0
    near = np.isfinite(prims.box).all(axis=1) & (np.abs(prims.box) < 1e6).all(axis=1)
    pick = np.flatnonzero(kinds & near)
    if not len(pick):
        pick = np.flatnonzero(near)
    k = r.choice(pick, n)
    # strictly inside, so that the aimed ray does meet the primitive's plane within it
    out = np.zeros((n, 3))
    a, b = r.uniform(0.05, 0.95, n), r.uniform(0.05, 0.95, n)
    for i in range(n):
        kk = k[i]
        if prims.kind[kk] == 0:
            out[i] = prims.c[kk]
        elif prims.kind[kk] == 1:
            um, uM, vm, vM, pos = prims.rect[kk]
            ax = prims.axis[kk] >> 1
            o1, o2 = [x for x in range(3) if x != ax]
            out[i, ax], out[i, o1], out[i, o2] = pos, um + a[i] * (uM - um), vm + b[i] * (vM - vm)
        else:
            s, t = a[i] * 0.9, b[i] * (1.0 - a[i]) * 0.9
            out[i] = prims.p[kk, 0] + s * prims.e1[kk] + t * prims.e2[kk]
    return out, k


def corrupted(name, o, d, r, root_box):
    """The rays (o, d) with the corruption of a CORRUPT class, or with the direction times 2^k for a SCALED class: (o, d)."""
    n = len(o)
    o, d = o.copy(), d.copy()
    one = r.integers(0, 3, n)            # the component a "one" class touches
    rows = np.arange(n)
    if name == "d_nan_all":
        d[:] = NAN
    elif name == "d_nan_one":
        d[rows, one] = NAN
    elif name == "o_nan_one":
        o[rows, one] = NAN
    elif name == "o_nan_all":
        o[:] = NAN
    elif name == "d_pinf_one":
        d[rows, one] = INF
    elif name == "d_ninf_one":
        d[rows, one] = -INF
    elif name == "o_pinf_one":
        o[rows, one] = INF
    elif name == "o_ninf_one":
        o[rows, one] = -INF
    elif name in ("o_pinf_d_pinf", "o_pinf_d_ninf"):
        o[rows, one] = INF
        d[rows, one] = INF if name == "o_pinf_d_pinf" else -INF
    elif name in ("d_pzero_inside", "d_nzero_inside"):
        b = np.asarray(root_box, dtype=np.float64)
        o = r.uniform(b[0::2], b[1::2], (n, 3))
        d[:] = 0.0 if name == "d_pzero_inside" else -0.0
        half = rows % 2 == 1             # every other ray: one component of the other sign
        d[rows[half], one[half]] = -0.0 if name == "d_pzero_inside" else 0.0
    elif name == "d_denormal_one":
        d[rows, one] = np.where(r.random(n) < 0.5, 5e-324, -5e-324)
    else:
        d = d * 2.0 ** SCALES[SCALED.index(name)]
    return o, d


def _class_rays(name, prims, base, r, root_box):
    """2 * RUN rays of the class from 2 * RUN base rays."""
    n = 2 * RUN
    o, d, aim = base.o.copy(), base.d.copy(), base.aim.copy()
    if name in CORRUPT:
        o, d = corrupted(name, o, d, r, root_box)
    elif name in SCALED:
        target, aim = _flat_targets(prims, r, n)
        o, d = corrupted(name, o, target - o, r, root_box)
    else:
        far = name in FAR_AXIS
        k = FAR[(FAR_AXIS if far else D_AXIS).index(name)]
        target, aim = _flat_targets(prims, r, n, facing_y=True)
        o = target.copy()
        o[:, 1] = target[:, 1] + (2.0 ** k if far else r.uniform(1.0, 8.0, n))
        d = np.zeros((n, 3))
        d[:, 1] = -2.0 ** k
    return o, d, aim


def corrupt_in_runs(o, d, root_box, run, seed=20251):
    """(o, d) repeated to len(CORRUPT + SCALED) * 3 * run + 7 rays and corrupted class by class: a run of `run` rays that begins
    at a multiple of `run`, then `run` rays of the class ray by ray between rays left as they are.  Returns (o, d, corrupt):
    corrupt[i] says whether ray i was touched."""
    names = CORRUPT + SCALED
    total = len(names) * 3 * run + 7
    idx = np.arange(total) % len(o)
    o, d = np.ascontiguousarray(o[idx], dtype=np.float64), np.ascontiguousarray(d[idx], dtype=np.float64)
    r = np.random.default_rng(seed)
    touched = np.zeros(total, dtype=bool)
    with np.errstate(all="ignore"):
        for c, name in enumerate(names):
            at = c * 3 * run
            i = np.concatenate([np.arange(at, at + run), np.arange(at + run, at + 3 * run, 2)])
            o[i], d[i] = corrupted(name, o[i], d[i], r, root_box)
            touched[i] = True
    return o, d, touched


def nonfinite_rays(scene, prims=None):
    """(Rays, spans): spans[class] = (the run's slice, the interleaved rays' slice); spans["ordinary"] the general rays
    between and behind them."""
    prims = prims if prims is not None else G.Prims(G.SCENES[scene]())
    r = np.random.default_rng(sum(ord(c) for c in scene) + 20250)
    n_cls = len(CLASSES)
    total = n_cls * 3 * RUN + TAIL
    base = G.rays_for(scene, "general", n_cls * 3 * RUN + TAIL, prims)
    finite = prims.box[np.isfinite(prims.box).all(axis=1) & (np.abs(prims.box) < 1e6).all(axis=1)]
    root_box = np.stack([finite[:, 0::2].min(axis=0), finite[:, 1::2].max(axis=0)], axis=1).reshape(-1)
    o, d, aim = base.o.copy(), base.d.copy(), base.aim.copy()
    spans, ordinary = {}, np.ones(total, dtype=bool)
    with np.errstate(all="ignore"):
        for c, name in enumerate(CLASSES):
            at = c * 3 * RUN
            run, mixed = slice(at, at + RUN), slice(at + RUN, at + 3 * RUN, 2)
            idx = np.concatenate([np.arange(total)[run], np.arange(total)[mixed]])
            co, cd, ca = _class_rays(name, prims, G.Rays(o[idx], d[idx], aim[idx]), r, root_box)
            o[idx], d[idx], aim[idx] = co, cd, ca
            ordinary[idx] = False
            spans[name] = (run, mixed)
    spans["ordinary"] = (ordinary,)
    assert total % RUN != 0
    return G.Rays(np.ascontiguousarray(o), np.ascontiguousarray(d), aim.astype(np.int64)), spans


def class_index(spans, name, n):
    """The indices of a class's rays in a batch of n."""
    return np.concatenate([np.arange(n)[s] for s in spans[name]])


def hot_triangles(prims, hot_objects):
    return [int(k) for k in hot_objects if prims.kind[int(k)] == 2]


def settled_against(prims, k, o, d):
    """test_hot_group.settled of Triangle::intersect's three numerators and den for triangle k and every ray."""
    p1, e1, e2 = (tuple(float(x) for x in a[k]) for a in (prims.p[:, 0], prims.e1, prims.e2))
    with np.errstate(all="ignore"):
        t = G.sub(o, p1)
        p = G.cross(d, e2)
        q = G.cross(t, e1)
        den = G.dot(p, e1)
        n0, n1, n2 = G.dot(q, e2), G.dot(p, t), G.dot(q, d)
    return settled(*(np.ascontiguousarray(x, dtype=np.float64) for x in (n0, n1, n2, den)))


def check_classes(scene, window, reading, rays, spans, t, obj, hot_objects=None):
    """Assert, on the second reading itself, that the classes show what they are made for.  window: a key of WINDOWS; t, obj:
    the reading's answer for `rays` under that window; hot_objects: the objects of the product's hot group (None: no group).
    Returns {class: hits of its 2 * RUN rays}."""
    n = len(rays.o)
    tmin, tmax = WINDOWS[window]
    o, d = G.vec(rays.o), G.vec(rays.d)
    root = reading.tree.box
    with np.errstate(all="ignore"):
        entered = G.aabb_intersect(root, o, d, tmin, tmax) & np.ones(n, dtype=bool)
    hits = {name: int((obj[class_index(spans, name, n)] >= 0).sum()) for name in CLASSES}
    assert not np.isnan(t).any() and (t[obj < 0] == 0.0).all()
    # a ray with an all-NaN direction or origin enters the root box (and every other one: each slab's NaN is ignored), and
    # hits nothing
    for name in ("d_nan_all", "o_nan_all"):
        i = class_index(spans, name, n)
        assert entered[i].all() and hits[name] == 0, (scene, window, name)
    for name in ("d_pzero_inside", "d_nzero_inside"):
        assert entered[class_index(spans, name, n)].all(), (scene, window, name)
    # an origin 2^160 or more away absorbs the scene: the root box has no thickness in t, and is never entered
    for name in FAR_AXIS:
        i = class_index(spans, name, n)
        assert not entered[i].any() and hits[name] == 0, (scene, window, name)
    if window == "t0_t1":
        for name in SCALED + D_AXIS:     # t is 2^-k times an ordinary one: outside (1e-6, 1e6)
            assert hits[name] == 0, (scene, window, name, hits[name])
    elif scene in HOT_SCENES:
        for name in SCALED + (D_AXIS if scene == "floor_spheres" else ()):
            assert hits[name] >= 32 * (2 * RUN) // 512, (scene, window, name, hits[name])
    if window in OPEN and scene in ("floor_spheres", "soup"):
        # spheres are lost once dot(d, d) overflows or underflows: no scaled ray with |k| >= 600 reports one
        sph = reading.prims.kind == 0
        for k in (600, 1000, -600, -1000):
            i = class_index(spans, f"scale_2^{k}", n)
            assert not sph[obj[i][obj[i] >= 0]].any(), (scene, window, k)
        i = class_index(spans, "scale_2^400", n)
        if scene == "soup":
            assert sph[obj[i][obj[i] >= 0]].any(), (scene, window)
    ordinary = spans["ordinary"][0]
    if window == "t0_t1":
        assert (obj[ordinary] >= 0).mean() >= 0.30, (scene, float((obj[ordinary] >= 0).mean()))
    if hot_objects is not None:
        tris = hot_triangles(reading.prims, hot_objects)
        if tris:
            _check_settled(scene, reading.prims, tris, o, d, spans, n)
    return hits


def _check_settled(scene, prims, tris, o, d, spans, n):
    """The hot group's shortcut (device_path.h hot_triangle_intersect) skips the divisions only if every lane of a wave is
    settled: at least two classes have an aligned run of 64 all of whose rays are settled against one triangle of the group, and
    at least two other classes have, in every aligned run of 64, a ray that is settled against none."""
    whole, never = [], []
    for name in CLASSES:
        run = spans[name][0]
        s = np.stack([settled_against(prims, k, G.take(o, run), G.take(d, run)) for k in tris])   # (triangles, RUN)
        waves = s.reshape(len(tris), RUN // 64, 64)
        if waves.all(axis=2).any():
            whole.append(name)
        elif (~s.any(axis=0)).reshape(RUN // 64, 64).any(axis=1).all():
            never.append(name)
    assert len(whole) >= 2 and len(never) >= 2, (scene, whole, never)
    return whole, never
