"""A second, independent reading of the ray queries of rayrs-lib/src/geometry.rs and bvh.rs, in plain numpy float64 written
from the Rust text, and the seeded ray families it is compared on (tests/test_second_reading_of_geometry_rs.py against the
oracle, tests/test_gpu_geometry_reading.py against the kernels).

Every expression is evaluated element by element, in the operand order of the Rust source: no np.cross, np.dot, einsum or
linalg (they reorder sums), nothing fused (numpy never contracts a * b + c).  Under np.errstate(all="ignore") every value is
then the IEEE value of the reference's expression -- NaN and infinities included -- so the comparisons are exact: no
tolerance and no ray left out.  f64::max / f64::min return the other operand when one is NaN: np.fmax / np.fmin.

A vector is a tuple of three arrays (or scalars): (x, y, z)."""
import math
from dataclasses import dataclass

import numpy as np

import test_second_reading_of_bvh_rs as B
from rayrs_amd import scenes
from rayrs_amd.api import Axis, BvhHeuristic, Emission, Material, Object
from test_bvh_builder import degenerate_objects

T0, T1 = 1e-6, 1e6
NR, DARK = Material.NoReflect(), Emission.Dark()
HEURISTICS = {"sah1000": BvhHeuristic.Sah(1000), "sah7": BvhHeuristic.Sah(7), "midpoint": BvhHeuristic.Midpoint}


# ---------------------------------------------------------------------------------------------------- vecmath.rs

def add(a, b):  # impl Add for Vector<f64>, vecmath.rs:716-728
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def sub(a, b):  # impl Sub, vecmath.rs:762-774
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def scale(a, s):  # impl Mul<f64> for Vector<f64>, vecmath.rs:614-622: each component times the scalar
    return (a[0] * s, a[1] * s, a[2] * s)


def dot(a, b):  # vecmath.rs:530-536: x*x' + y*y' + z*z', summed left to right
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def cross(a, b):  # vecmath.rs:562-574
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def mag(a):  # vecmath.rs:517-523: mag2().sqrt(), mag2 = dot(self, self)
    return np.sqrt(dot(a, a))


def unit(a):  # vecmath.rs:525-527 with Div<f64> (:690-698): multiplies by the reciprocal 1 / mag, it does not divide
    return scale(a, 1.0 / mag(a))


def point(o, d, t):  # Ray::point, lib.rs:41-43: origin + direction * t
    return add(o, scale(d, t))


def vec(a):
    """(n, 3) array -> vector of three (n,) arrays"""
    a = np.asarray(a, dtype=np.float64)
    return (a[..., 0], a[..., 1], a[..., 2])


def take(v, m):
    return (v[0][m], v[1][m], v[2][m])


# ---------------------------------------------------------------------------------------------------- geometry.rs

def sphere_intersect(radius, c, o, d):
    """Sphere::new keeps radius * radius (geometry.rs:96-102); Sphere::intersect, :106-132.  Returns (Some?, t, t1):
    quirk (b) -- t1 in [0, tmin) is Some(t1), which the leaf then rejects, so the far side t2 is lost."""
    radius2 = radius * radius
    odiff = sub(o, c)
    a = dot(d, d)
    b = 2.0 * dot(d, odiff)
    cc = dot(odiff, odiff) - radius2
    desc = b * b - 4.0 * a * cc
    t1 = (-b - np.sqrt(desc)) / (2.0 * a)
    t2 = (-b + np.sqrt(desc)) / (2.0 * a)
    some = (desc > 0.0) & ~((t1 < 0.0) & (t2 < 0.0))
    return some, np.where(t1 < 0.0, t2, t1), t1


def sphere_normal(c, p):  # geometry.rs:134-136
    return unit(sub(p, c))


def range_contains(start, end, x):  # core::ops::Range::contains: start <= x && x < end
    return (start <= x) & (x < end)


def plane_intersect(axis, umin, umax, vmin, vmax, pos, o, d):
    """Plane::intersect, geometry.rs:229-271: X | XRev test d.x and (y, z), Y | YRev d.y and (x, z), Z | ZRev d.z and (x, y)."""
    ax = axis >> 1
    t = (pos - o[ax]) / d[ax]
    p = point(o, d, t)
    u, v = {0: (p[1], p[2]), 1: (p[0], p[2]), 2: (p[0], p[1])}[ax]
    return (d[ax] != 0.0) & range_contains(umin, umax, u) & range_contains(vmin, vmax, v), t


def plane_normal(axis):  # geometry.rs:273-282
    n = [0.0, 0.0, 0.0]
    n[axis >> 1] = -1.0 if axis & 1 else 1.0
    return tuple(n)


def triangle_new(p1, p2, p3):
    """Triangle::new, geometry.rs:341-354: (e1, e2, normal)."""
    e1 = sub(p2, p1)
    e2 = sub(p3, p1)
    return e1, e2, unit(cross(e1, e2))


def triangle_intersect(p1, e1, e2, o, d):
    """Triangle::intersect (Moeller-Trumbore), geometry.rs:359-375.  Returns (Some?, t, u, v): a NaN quotient fails
    every compare, so it is Some(NaN) -- which the leaf's t > tmin then rejects."""
    t = sub(o, p1)
    p = cross(d, e2)
    q = cross(t, e1)
    den = dot(p, e1)
    dd = dot(q, e2) / den
    u = dot(p, t) / den
    v = dot(q, d) / den
    return ~((dd < 0.0) | (u < 0.0) | (v < 0.0) | (u + v > 1.0)), dd, u, v


def aabb_intersect(box, o, d, tmin, tmax):
    """AxisAlignedBoundingBox::intersect, geometry.rs:458-513.  box = (xmin, xmax, ymin, ymax, zmin, zmax)."""
    ok = True
    for k in range(3):
        hi_k = box[2 * k + 1] - o[k]
        lo_k = box[2 * k] - o[k]
        inv = 1.0 / d[k]
        neg = inv < 0.0
        tk0 = np.where(neg, hi_k * inv, lo_k * inv)
        tk1 = np.where(neg, lo_k * inv, hi_k * inv)
        tmin = np.fmax(tmin, tk0)  # f64::max: a NaN operand is ignored
        tmax = np.fmin(tmax, tk1)
        ok = ok & ~(tmax <= tmin)  # (the reference returns here; the later axes cannot turn false into true)
    return ok


# ---------------------------------------------------------------------------------------------------- primitives

class Prims:
    """The primitives of a scene description in insertion order (a mesh is its triangles), with what Triangle::new
    keeps, as arrays indexed by object: the object index is the one rayrs_test_intersect and the oracle report."""

    def __init__(self, objs):
        self.list = B.singles(objs)
        n = len(self.list)
        self.kind = np.array([{"sphere": 0, "plane": 1, "triangle": 2}[o.kind] for o in self.list])
        self.radius = np.array([o.radius for o in self.list])
        self.c = np.array([o.origin for o in self.list], dtype=np.float64).reshape(n, 3)
        self.axis = np.array([o.axis for o in self.list])
        self.rect = np.array([(o.umin, o.umax, o.vmin, o.vmax, o.pos) for o in self.list]).reshape(n, 5)
        self.p = np.array([o.p for o in self.list], dtype=np.float64).reshape(n, 3, 3)
        with np.errstate(all="ignore"):
            self.e1, self.e2, self.normal = (np.stack(x, axis=-1) for x in
                                             triangle_new(vec(self.p[:, 0]), vec(self.p[:, 1]), vec(self.p[:, 2])))
        self.box = np.array([B.bbox_of(o) for o in self.list], dtype=np.float64).reshape(n, 6)

    def __len__(self):
        return len(self.kind)

    def intersect(self, k, o, d):
        """Hittable::intersect of object k[i] with ray i (k: array, or one index for every ray): (Some?, t, extra) with
        extra = {"u", "v"} for triangles and {"t1"} for spheres (NaN where it does not apply)."""
        n = len(o[0])
        k = np.broadcast_to(np.asarray(k), (n,))
        some, t = np.zeros(n, dtype=bool), np.full(n, np.nan)
        extra = {"u": np.full(n, np.nan), "v": np.full(n, np.nan), "t1": np.full(n, np.nan)}
        for kind in (0, 1, 2):
            m = self.kind[k] == kind
            if not m.any():
                continue
            km, om, dm = k[m], take(o, m), take(d, m)
            if kind == 0:
                s, tt, t1 = sphere_intersect(self.radius[km], vec(self.c[km]), om, dm)
                extra["t1"][m] = t1
            elif kind == 1:
                s, tt = np.zeros(len(km), dtype=bool), np.zeros(len(km))
                for ax in range(6):
                    a = self.axis[km] == ax
                    if a.any():
                        r = self.rect[km[a]].T
                        s[a], tt[a] = plane_intersect(ax, r[0], r[1], r[2], r[3], r[4], take(om, a), take(dm, a))
            else:
                s, tt, u, v = triangle_intersect(vec(self.p[km, 0]), vec(self.e1[km]), vec(self.e2[km]), om, dm)
                extra["u"][m], extra["v"][m] = u, v
            some[m], t[m] = s, tt
        return some, t, extra


# ---------------------------------------------------------------------------------------------------- bvh.rs

class Reading:
    """Bvh::build (the tree of test_second_reading_of_bvh_rs.build) and BvhTree::intersect (bvh.rs:391-415) with the fold
    and RayIntersection::update (:50-72), vectorised over rays: each Node tests its box for the rays that reached it and
    passes on those that entered."""

    def __init__(self, objs, heuristic):
        self.prims = Prims(objs)
        items = [(i, tuple(float(x) for x in self.prims.box[i])) for i in range(len(self.prims))]
        splits = heuristic[1] if heuristic[0] == "sah" else 0
        self.tree = B.build(items, splits, [], [])

    def intersect(self, o, d, tmin=T0, tmax=T1):
        """(t, object) per ray: object -1 for a Miss (t is then 0).  Also sets self.stats: flat_entered (Node boxes of zero
        extent on some axis that a ray entered) and tie (rays whose two best accepted hits have equal t)."""
        o, d = vec(o), vec(d)
        n = len(o[0])
        self._tie_t = np.full(n, np.inf)
        self._flat = 0
        self._tmin, self._tmax = tmin, tmax
        with np.errstate(all="ignore"):
            hit, t, obj = self._visit(self.tree, o, d, np.arange(n))
        obj = np.where(hit, obj, -1)
        t = np.where(hit, t, 0.0)
        self.stats = {"flat_entered": self._flat, "tie": hit & (self._tie_t == t)}
        return t, obj

    def _visit(self, node, o, d, ids):
        n = len(ids)
        if isinstance(node, B.LeafNode):  # bvh.rs:404-413
            some, t, _ = self.prims.intersect(node.object, o, d)
            return some & (t > self._tmin) & (t < self._tmax), t, np.full(n, node.object)
        hit, t, obj = np.zeros(n, dtype=bool), np.zeros(n), np.full(n, -1)
        entered = aabb_intersect(node.box, o, d, self._tmin, self._tmax) & np.ones(n, dtype=bool)  # bvh.rs:394
        if not entered.any():
            return hit, t, obj
        b = node.box
        if b[0] == b[1] or b[2] == b[3] or b[4] == b[5]:
            self._flat += int(entered.sum())
        o2, d2, ids2 = take(o, entered), take(d, entered), ids[entered]
        # children.iter().fold(Miss, |acc, child| acc.update(child.intersect(..), tmin)), bvh.rs:395-399
        ah, at, ao = np.zeros(len(ids2), dtype=bool), np.zeros(len(ids2)), np.full(len(ids2), -1)
        for child in node.children:
            ch, ct, co = self._visit(child, o2, d2, ids2)
            tie = ah & ch & (ct == at)
            self._tie_t[ids2[tie]] = np.fmin(self._tie_t[ids2[tie]], at[tie])
            # update (bvh.rs:50-72): (Miss, Hit) -> the new one; (Hit, Hit) -> the new one iff t > tmin && t < t_old
            new = ch & (~ah | ((ct > self._tmin) & (ct < at)))
            at = np.where(new, ct, at)
            ao = np.where(new, co, ao)
            ah = ah | ch
        hit[entered], t[entered], obj[entered] = ah, at, ao
        return hit, t, obj


# ---------------------------------------------------------------------------------------------------- scenes

def grid_soup():
    """Spheres, rectangles and dyadic triangles on an integer grid -- a fifth of them axis-aligned in a grid plane --,
    exact duplicates of sixty of them inserted after the originals, and one sphere off the grid."""
    r = np.random.default_rng(11)
    objs = []
    for i in range(300):
        c = r.integers(-6, 7, 3).astype(float)
        if i % 3 == 0:
            objs.append(Object.sphere(float(r.integers(1, 3)) * 0.5, c, NR, DARK))
        elif i % 3 == 1:
            objs.append(Object.plane(int(r.integers(0, 6)), c[0], c[0] + 2.0, c[1], c[1] + 1.0, c[2], NR, DARK))
        else:
            e = r.integers(-2, 3, (2, 3)) * 0.5
            if i % 5 == 0:
                e[:, int(r.integers(0, 3))] = 0.0  # in a grid plane
            if not np.cross(e[0], e[1]).any():
                e = np.array([[1.0, 0.0, 0.0], [0.0, 0.5, 0.0]])
            objs.append(Object.triangle(c, c + e[0], c + e[1], NR, DARK))
    objs += [objs[int(k)] for k in r.choice(len(objs), 60, replace=False)]
    objs.append(Object.sphere(0.1, (9.0, 9.0, 9.0), NR, DARK))  # a box bound f32 cannot hold: the f64 layout
    return objs


def floor_spheres():
    """The floor and sixty spheres of test_gpu_hot_group.test_a_group_of_spheres_and_a_rectangle_can_be_the_hot_group."""
    r = np.random.default_rng(3)
    grey = Material.LambertianDiffuse((0.7, 0.7, 0.7))
    objs = [Object.plane(Axis.Y, -25.0, 25.0, -25.0, 25.0, 0.0, grey, Emission.Dark())]
    for i in range(60):
        c = r.uniform(-2.0, 2.0, 3)
        c[1] = abs(c[1]) + 0.3
        objs.append(Object.sphere(0.2, c, Material.Reflect((0.9, 0.9, 0.9)) if i % 2 else grey, Emission.Dark()))
    return objs


def layers():
    """Layers eight apart, each four objects in one grid plane (rectangles and triangles flat in y, x or z): the bottom
    Nodes' boxes have zero extent across their layer -- a ray that crosses such a layer never enters them.  In two layers
    of three one triangle leans out of the plane, which gives their Node thickness."""
    objs = []
    for k in range(12):
        ax = k % 3
        pos = 8.0 * k
        for j in range(4):
            u0, v0 = float(2 * (j % 2)), float(2 * (j // 2))
            if j % 2 == 0:
                objs.append(Object.plane(2 * ax + (k // 3) % 2, u0, u0 + 1.5, v0, v0 + 1.5, pos, NR, DARK))
            else:
                q = [[u0, v0], [u0 + 1.5, v0], [u0, v0 + 1.5]]
                pts = []
                for uv in q:
                    p = [0.0, 0.0, 0.0]
                    p[ax] = pos
                    o1, o2 = [a for a in range(3) if a != ax]
                    p[o1], p[o2] = uv
                    pts.append(p)
                if j == 3 and k % 3:
                    pts[2][ax] += 0.5
                objs.append(Object.triangle(*pts, NR, DARK))
    return objs


def ties():
    """A 2 x 2 rectangle at z = 0 and the two triangles that tile it, each triangle twice; exact duplicate spheres and
    rectangles elsewhere; shuffled, so that depth-first order is not insertion order."""
    objs = [Object.plane(Axis.Z, 0.0, 2.0, 0.0, 2.0, 0.0, NR, DARK),
            Object.triangle((0.0, 0.0, 0.0), (2.0, 0.0, 0.0), (0.0, 2.0, 0.0), NR, DARK),
            Object.triangle((2.0, 2.0, 0.0), (0.0, 2.0, 0.0), (2.0, 0.0, 0.0), NR, DARK)]
    objs += objs[1:3]
    for x in (-4.0, 4.0):
        objs += [Object.sphere(1.0, (x, 1.0, 1.0), NR, DARK)] * 2
        objs += [Object.plane(Axis.XRev, -1.0, 3.0, -1.0, 3.0, x + 2.0, NR, DARK)] * 2
    perm = np.random.default_rng(6).permutation(len(objs))
    return [objs[i] for i in perm]


NEAR_FAR = {"t0": T0, "above_t0": float(np.nextafter(T0, np.inf)), "below_t1": float(np.nextafter(T1, 0.0)), "t1": T1}


def near_far(where):
    """A 2 x 2 rectangle at y = NEAR_FAR[where] and a sphere beside it that gives the root box thickness around it
    (a lone rectangle's flat root box is never entered)."""
    return [Object.plane(Axis.Y, -1.0, 1.0, -1.0, 1.0, NEAR_FAR[where], NR, DARK),
            Object.sphere(3.0, (5.0, 0.0, 0.0), NR, DARK)]


SCENES = {
    "mesh1280_light": lambda: scenes.mesh_scene(3, area_light=True)[1],
    "mesh5120": lambda: scenes.mesh_scene(4)[1],
    "soup": lambda: B.soup()[1],
    "grid_soup": grid_soup,
    "degenerate": degenerate_objects,
    "floor_spheres": floor_spheres,
    "layers": layers,
    "ties": ties,
    **{"near_far_" + k: (lambda k=k: near_far(k)) for k in NEAR_FAR},
}


# ---------------------------------------------------------------------------------------------------- ray families

@dataclass
class Rays:
    o: np.ndarray    # (n, 3)
    d: np.ndarray    # (n, 3)
    aim: np.ndarray  # (n,) the object each ray is put to in the per-primitive comparison


def _around(prims, r, n):
    """test_gpu_functions._rays on the scene's scale: origins around the scene, targets inside the box of a random
    object, a quarter of the directions random, some components exactly zero."""
    near = np.flatnonzero(np.isfinite(prims.box).all(axis=1) & (np.abs(prims.box) < 1e6).all(axis=1))
    finite = prims.box[near]
    lo, hi = finite[:, 0::2].min(axis=0), finite[:, 1::2].max(axis=0)
    ext = np.maximum(hi - lo, 1.0)
    o = r.uniform(lo - 0.5 * ext, hi + 0.5 * ext, (n, 3))
    b = prims.box[r.choice(near, n)]
    target = r.uniform(b[:, 0::2], b[:, 1::2])
    d = target - o
    d[: n // 4] = r.normal(size=(n // 4, 3))
    d[n // 4: n // 4 + n // 64, 0] = 0.0
    d[n // 4 + n // 64: n // 4 + n // 32, 1] = 0.0
    d[n // 4 + n // 32: n // 4 + 3 * n // 64, 2] = -0.0
    return o, d


def _point_on(prims, k, r):
    """A point on object k[i] (or just beside it)."""
    n = len(k)
    out = np.zeros((n, 3))
    a, b = r.uniform(-0.1, 1.1, n), r.uniform(-0.1, 1.1, n)
    for i in range(n):
        kk = k[i]
        if prims.kind[kk] == 0:
            v = r.normal(size=3)
            out[i] = prims.c[kk] + v / np.linalg.norm(v) * prims.radius[kk] * (1.0 + r.uniform(-0.05, 0.05))
        elif prims.kind[kk] == 1:
            um, uM, vm, vM, pos = prims.rect[kk]
            ax = prims.axis[kk] >> 1
            o1, o2 = [x for x in range(3) if x != ax]
            out[i, ax], out[i, o1], out[i, o2] = pos, um + a[i] * (uM - um), vm + b[i] * (vM - vm)
        else:
            s, t = a[i], b[i] * (1.0 - a[i])
            out[i] = prims.p[kk, 0] + s * prims.e1[kk] + t * prims.e2[kk]
    return out


def general(prims, seed, n):
    r = np.random.default_rng(seed)
    o, d = _around(prims, r, n)
    return Rays(o, d, r.integers(0, len(prims), n))


def grid(prims, seed, n):
    """Integer and half-integer origins; half the rays aimed at dyadic points of a triangle's edges and vertices (a third
    of those from an origin in the triangle's own grid plane, where it has one), half with direction components in
    {-2, ..., 2}, some of them -0.0."""
    r = np.random.default_rng(seed)
    tris = np.flatnonzero(prims.kind == 2)
    o = r.integers(-8, 9, (n, 3)) + r.integers(0, 2, (n, 3)) * 0.5
    aim = r.choice(tris, n)
    h = n // 2
    edge = r.integers(0, 3, h)
    s = r.integers(0, 5, h)[:, None] * 0.25
    p1, p2, p3 = prims.p[aim[:h], 0], prims.p[aim[:h], 1], prims.p[aim[:h], 2]
    a = np.where((edge == 0)[:, None], p2, np.where((edge == 1)[:, None], p1, p1))
    b = np.where((edge == 0)[:, None], p3, np.where((edge == 1)[:, None], p2, p3))
    target = a + (b - a) * s
    for i in range(0, h, 3):  # an origin in the triangle's grid plane
        flat = np.flatnonzero((prims.p[aim[i], 0] == prims.p[aim[i], 1]) & (prims.p[aim[i], 0] == prims.p[aim[i], 2]))
        if len(flat):
            o[i, flat[0]] = prims.p[aim[i], 0, flat[0]]
    d = np.zeros((n, 3))
    d[:h] = target - o[:h]
    d[h:] = r.integers(-2, 3, (n - h, 3)).astype(float)
    d[(d == 0).all(axis=1)] = (1.0, 0.0, 0.0)
    m = (np.arange(n) % 7 == 3) & (np.arange(n) >= h)
    d[m] = np.where(d[m] == 0.0, -0.0, d[m])  # -0.0 for the zero components of a seventh of them
    return Rays(o, d, aim)


def in_plane(prims, seed, n):
    """Rays in a rectangle's or a triangle's plane: for a rectangle and for a triangle flat in a grid plane the origin's
    coordinate is exactly the plane's and the direction's component exactly (+-)0 -- also the plane of a Node's box of
    zero extent; for any other triangle an origin and a target in its plane, as computed."""
    r = np.random.default_rng(seed)
    rects, tris = np.flatnonzero(prims.kind == 1), np.flatnonzero(prims.kind == 2)
    aim = r.choice(tris, n) if len(tris) else r.choice(rects, n)
    if len(rects):
        pick = r.random(n) < 0.3
        aim[pick] = r.choice(rects, int(pick.sum()))
    target = _point_on(prims, aim, r)
    o = np.zeros((n, 3))
    for i in range(n):
        k = aim[i]
        if prims.kind[k] == 1:
            ax = prims.axis[k] >> 1
        else:
            flat = np.flatnonzero((prims.p[k, 0] == prims.p[k, 1]) & (prims.p[k, 0] == prims.p[k, 2]))
            ax = flat[0] if len(flat) else -1
        if ax >= 0:
            o[i] = target[i] + r.uniform(-3.0, 3.0, 3)
            o[i, ax] = target[i, ax]
        else:
            o[i] = _point_on(prims, [k], r)[0] * 1.0
            o[i] = o[i] + (o[i] - target[i]) * r.uniform(0.5, 4.0)
    d = target - o
    flip = r.random(n) < 0.5
    d[flip] = np.where(d[flip] == 0.0, -0.0, d[flip])  # zero components as -0.0
    d[(d == 0).all(axis=1)] = (1.0, 0.0, 0.0)
    return Rays(o, d, aim)


def on_surface(prims, seed, n):
    """Rays that start where an earlier ray hit an object, as bounce rays do (Ray::point of the hit's t), into random
    directions -- spheres first where the scene has any."""
    r = np.random.default_rng(seed)
    spheres = np.flatnonzero(prims.kind == 0)
    os_, ds_, ks_ = [], [], []
    got = 0
    while got < n:
        m = 2 * (n - got) + 64
        k = np.where(r.random(m) < 0.7, r.choice(spheres, m), r.integers(0, len(prims), m)) if len(spheres) else \
            r.integers(0, len(prims), m)
        target = _point_on(prims, k, r)
        o = target + r.normal(size=(m, 3)) * (1.0 + np.abs(target).max(axis=1, keepdims=True) * 0.1)
        d = target - o
        with np.errstate(all="ignore"):
            some, t, _ = prims.intersect(k, vec(o), vec(d))
            keep = some & np.isfinite(t) & (t > 0.0)
            p = np.stack(point(vec(o[keep]), vec(d[keep]), t[keep]), axis=-1)
        nd = r.normal(size=p.shape)
        os_.append(p), ds_.append(nd), ks_.append(k[keep])
        got += len(p)
    return Rays(np.concatenate(os_)[:n], np.concatenate(ds_)[:n], np.concatenate(ks_)[:n])


def near_far_rays(prims, seed, n):
    """Straight up from y = 0 through the rectangle (t is exactly its position), through its edges and beside it, and
    rays around the scene."""
    r = np.random.default_rng(seed)
    h = n // 2
    o = np.zeros((n, 3))
    o[:h, 0], o[:h, 2] = r.integers(-6, 7, (2, h)) * 0.25
    d = np.zeros((n, 3))
    d[:h, 1] = 1.0
    o[h:], d[h:] = _around(prims, r, n - h)
    return Rays(o, d, np.where(np.arange(n) < h, 0, r.integers(0, len(prims), n)))


def ties_rays(prims, seed, n):
    """Dyadic origins above the tiled rectangle, dyadic targets on it; and rays around the scene."""
    r = np.random.default_rng(seed)
    h = 3 * n // 4
    o = np.zeros((n, 3))
    o[:h] = r.integers(-8, 9, (h, 3)) * 0.5
    o[:h, 2] = r.integers(1, 9, h) * 0.5
    target = np.zeros((h, 3))
    target[:, :2] = r.integers(0, 17, (h, 2)) * 0.125
    d = np.zeros((n, 3))
    d[:h] = target - o[:h]
    o[h:], d[h:] = _around(prims, r, n - h)
    return Rays(o, d, r.integers(0, len(prims), n))


def extreme(prims, seed, n):
    """At the point, the segment and the tiny sphere of degenerate_objects(), around the scene, and with subnormal
    coordinates: origins and direction components of 1e-310 and 5e-324.  (A direction that comes out all zero is replaced:
    zero, NaN, infinite and far-scaled rays are tests/_nonfinite_rays.py's.)"""
    r = np.random.default_rng(seed)
    o, d = _around(prims, r, n)
    q = n // 4
    targets = np.array([[0.5, 1.0, -0.25], [1.5, 1.0, -0.25], [-1.0, 1.0, 1.0], [0.25, 2.0, 0.25]])
    d[:q] = targets[r.integers(0, 4, q)] - o[:q]
    sub = np.array([0.0, 5e-324, -5e-324, 1e-310, -1e-310, 2.5e-308])
    s0, s1 = q, 2 * q
    o[s0:s1] = np.where(r.random((q, 3)) < 0.5, sub[r.integers(0, 6, (q, 3))], o[s0:s1])
    o[s0:s1, 1] = np.abs(o[s0:s1, 1]) + np.where(r.random(q) < 0.5, 1e-310, 1.0)
    d[s0:s1] = np.where(r.random((q, 3)) < 0.3, sub[r.integers(0, 6, (q, 3))], d[s0:s1])
    d[(d == 0).all(axis=1)] = (0.0, -1.0, 0.0)
    return Rays(o, d, r.integers(0, len(prims), n))


FAMILIES = {"general": general, "grid": grid, "in_plane": in_plane, "on_surface": on_surface, "near_far": near_far_rays,
            "ties": ties_rays, "extreme": extreme}

# (scene, family) cases: each family on the scenes it is made for
CASES = [(s, f) for s in ("mesh1280_light", "mesh5120", "soup") for f in ("general", "in_plane", "on_surface")] + \
        [("grid_soup", "grid"), ("grid_soup", "general"), ("grid_soup", "in_plane"), ("degenerate", "extreme"),
         ("floor_spheres", "general"), ("floor_spheres", "on_surface"), ("layers", "in_plane"), ("layers", "general"),
         ("ties", "ties")] + \
        [("near_far_" + k, "near_far") for k in NEAR_FAR]

N_RAYS = 40000  # the unit the families' conditions are stated in


def rays_for(scene, family, n=N_RAYS, prims=None):
    prims = prims if prims is not None else Prims(SCENES[scene]())
    seed = sum(ord(c) for c in scene + family)
    with np.errstate(all="ignore"):
        rays = FAMILIES[family](prims, seed, n)
    return Rays(np.ascontiguousarray(rays.o, dtype=np.float64), np.ascontiguousarray(rays.d, dtype=np.float64),
                np.asarray(rays.aim, dtype=np.int64))


def scene_rays(scene, n=N_RAYS):
    """Every family of the scene's cases, concatenated, and where each one lies."""
    prims = Prims(SCENES[scene]())
    parts, spans, at = [], {}, 0
    for s, f in CASES:
        if s == scene:
            r = rays_for(s, f, n, prims)
            parts.append(r)
            spans[f] = slice(at, at + len(r.o))
            at += len(r.o)
    return Rays(np.concatenate([p.o for p in parts]), np.concatenate([p.d for p in parts]),
                np.concatenate([p.aim for p in parts])), spans


# ---------------------------------------------------------------------------------------------------- the edges

def check_family_edges(scene, family, reading, rays, t, obj, tie, flat_entered):
    """Assert, on the second reading itself, that the family shows the edge it is made for (per N_RAYS rays; thresholds
    are conditions on the inputs, set well below what these generators give).  t, obj, tie: the whole query's reading
    for these rays; flat_entered: Node boxes of zero extent entered by them."""
    n = len(rays.o)
    need = lambda x: math.ceil(x * n / N_RAYS)
    prims = reading.prims
    with np.errstate(all="ignore"):
        some, pt, ex = prims.intersect(rays.aim, vec(rays.o), vec(rays.d))
    hits = obj >= 0
    with np.errstate(all="ignore"):
        _check_edges(scene, family, prims, rays, some, pt, ex, hits, t, obj, tie, flat_entered, need)


def _check_edges(scene, family, prims, rays, some, pt, ex, hits, t, obj, tie, flat_entered, need):
    if family in ("general", "extreme"):
        assert hits.mean() >= 0.30, (scene, family, hits.mean())
    if family == "grid":
        tri = prims.kind[rays.aim] == 2
        nan_q = tri & (np.isnan(pt) | np.isnan(ex["u"]) | np.isnan(ex["v"]))
        uv1 = tri & some & (ex["u"] + ex["v"] == 1.0)
        on0 = tri & some & ((ex["u"] == 0.0) | (ex["v"] == 0.0))
        assert uv1.sum() >= need(1000) and nan_q.sum() >= need(100) and on0.sum() >= need(10), \
            (scene, int(uv1.sum()), int(nan_q.sum()), int(on0.sum()))
    if family == "in_plane":
        if scene == "layers":
            assert flat_entered >= need(20), (scene, flat_entered)
    if family == "on_surface" and (prims.kind == 0).any():
        t1 = ex["t1"]
        lost = (prims.kind[rays.aim] == 0) & some & (t1 >= 0.0) & (t1 < T0)
        assert lost.sum() >= need(100), (scene, int(lost.sum()))
    if family == "near_far":
        where = scene[len("near_far_"):]
        pos = NEAR_FAR[where]
        at = (rays.aim == 0) & some & (pt == pos)
        assert at.sum() >= need(100), (scene, int(at.sum()))
        if where in ("t0", "t1"):   # bvh.rs:406: t > tmin && t < tmax -- the hit at exactly T0 / T1 is not accepted
            assert not (obj[at] == 0).any()
        else:
            assert (obj[at] == 0).all() and (t[at] == pos).all()
    if family == "ties":
        assert tie.sum() >= need(100), (scene, int(tie.sum()))
