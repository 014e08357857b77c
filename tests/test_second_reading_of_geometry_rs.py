"""The second reading of the ray queries (tests/_geometry_reading.py: geometry.rs's Sphere / Plane / Triangle / box tests and
bvh.rs's BvhTree::intersect, in numpy written from the Rust text) against the oracle, bit for bit, with no tolerance and no
ray left out: per primitive on every ray family, and as whole queries on every scene under three builders -- against the
oracle's recursion (traversal 0) and against its walk of the records the kernels read (traversal 2 on a host-only product
scene, with the hot group where the scene has one).  Each family first shows, on the reading itself, the edge it is made
for (_geometry_reading.check_family_edges), so that none of them can quietly stop testing it."""
import ctypes as C
import functools

import numpy as np
import pytest

import _geometry_reading as G
import _oracle
import rayrs_amd
from rayrs_amd import procedural

HDRI = procedural.make_hdri(8, 4)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def scene_rays(scene):
    return G.scene_rays(scene)


@functools.lru_cache(maxsize=None)
def _orc():
    """The oracle's per-primitive entry points with raw-pointer arguments (one call per ray)."""
    L = C.CDLL(_oracle.LIB_PATH)
    vp, dbl = C.c_void_p, C.c_double
    f = {n: L[n] for n in ("orc_sphere_intersect", "orc_plane_intersect", "orc_triangle_intersect", "orc_aabb_intersect",
                           "orc_triangle_normal")}
    f["orc_sphere_intersect"].argtypes = [dbl, vp, vp, vp, vp]
    f["orc_plane_intersect"].argtypes = [C.c_int] + [dbl] * 5 + [vp, vp, vp]
    f["orc_triangle_intersect"].argtypes = [vp] * 6
    f["orc_aabb_intersect"].argtypes = [vp, vp, vp, dbl, dbl]
    f["orc_triangle_normal"].argtypes = [vp] * 4
    f["orc_triangle_normal"].restype = None
    return f


def oracle_primitive(prims, aim, o, d):
    """orc_*_intersect of object aim[i] with ray i, and orc_aabb_intersect of the object's own box: (Some?, t, entered)."""
    f = _orc()
    n = len(o)
    some, t, boxed = np.zeros(n, dtype=bool), np.zeros(n), np.zeros(n, dtype=bool)
    tt = np.zeros(1)
    po, pd, pt = o.ctypes.data, d.ctypes.data, tt.ctypes.data
    c, p, box = np.ascontiguousarray(prims.c), np.ascontiguousarray(prims.p), np.ascontiguousarray(prims.box)
    pc, pp, pb = c.ctypes.data, p.ctypes.data, box.ctypes.data
    sph, pln, tri, aab = f["orc_sphere_intersect"], f["orc_plane_intersect"], f["orc_triangle_intersect"], f["orc_aabb_intersect"]
    for i in range(n):
        k = int(aim[i])
        oi, di = po + 24 * i, pd + 24 * i
        kind = prims.kind[k]
        tt[0] = 0.0
        if kind == 0:
            s = sph(float(prims.radius[k]), pc + 24 * k, oi, di, pt)
        elif kind == 1:
            r = prims.rect[k]
            s = pln(int(prims.axis[k]), float(r[0]), float(r[1]), float(r[2]), float(r[3]), float(r[4]), oi, di, pt)
        else:
            s = tri(pp + 72 * k, pp + 72 * k + 24, pp + 72 * k + 48, oi, di, pt)
        some[i], t[i] = s != 0, tt[0]
        boxed[i] = aab(pb + 48 * k, oi, di, G.T0, G.T1) != 0
    return some, t, boxed


@pytest.mark.parametrize("scene,family", G.CASES, ids=[f"{s}-{f}" for s, f in G.CASES])
def test_each_primitive_test_is_the_oracles(scene, family):
    """Sphere / Plane / Triangle::intersect (the hit flag and the bits of t where there is one) and the box test of the
    object's own box, for every ray of the family against the object it is put to."""
    rays, spans = scene_rays(scene)
    sl = spans[family]
    o, d, aim = np.ascontiguousarray(rays.o[sl]), np.ascontiguousarray(rays.d[sl]), rays.aim[sl]
    prims = G.Prims(G.SCENES[scene]())
    with np.errstate(all="ignore"):
        some, t, _ = prims.intersect(aim, G.vec(o), G.vec(d))
        boxed = G.aabb_intersect(tuple(prims.box[aim].T), G.vec(o), G.vec(d), G.T0, G.T1)
    osome, ot, oboxed = oracle_primitive(prims, aim, o, d)
    assert np.array_equal(some, osome)
    assert np.array_equal(bits(t[some]), bits(ot[some]))
    assert np.array_equal(boxed, oboxed)
    assert some.sum() > 0 and boxed.sum() > 0


def test_the_per_primitive_cases_cover_every_kind_and_plane_axis():
    kinds, axes, flat_boxes = set(), set(), 0
    for scene, family in G.CASES:
        rays, spans = scene_rays(scene)
        prims = G.Prims(G.SCENES[scene]())
        aim = rays.aim[spans[family]]
        kinds |= set(prims.kind[aim].tolist())
        axes |= set(prims.axis[aim][prims.kind[aim] == 1].tolist())
        b = prims.box[aim]
        flat_boxes += int(((b[:, 0] == b[:, 1]) | (b[:, 2] == b[:, 3]) | (b[:, 4] == b[:, 5])).sum())
    assert kinds == {0, 1, 2} and axes == set(range(6)) and flat_boxes > 1000


def test_triangle_new_is_the_oracles():
    """Triangle::new's normal (geometry.rs:344-351: e1 x e2, times the reciprocal of its length) on every triangle of
    the scenes, degenerate ones included (their normal is NaN on both sides)."""
    f = _orc()["orc_triangle_normal"]
    out = np.zeros(3)
    checked = 0
    for scene in G.SCENES:
        prims = G.Prims(G.SCENES[scene]())
        p = np.ascontiguousarray(prims.p)
        for k in np.flatnonzero(prims.kind == 2).tolist():
            f(p.ctypes.data + 72 * k, p.ctypes.data + 72 * k + 24, p.ctypes.data + 72 * k + 48, out.ctypes.data)
            assert np.array_equal(bits(out), bits(prims.normal[k])) or \
                (np.isnan(out).all() and np.isnan(prims.normal[k]).all()), (scene, k)
            checked += 1
    assert checked > 6000


@pytest.mark.parametrize("heur", list(G.HEURISTICS), ids=list(G.HEURISTICS))
@pytest.mark.parametrize("scene", list(G.SCENES))
def test_whole_queries_are_the_oracles(scene, heur):
    """BvhTree::intersect for every ray of the scene's families: the reading's recursion, the oracle's recursion and the
    oracle's walk of the product's own records (the gate tree, the hot group beside it where there is one) agree on the
    object everywhere and on the bits of t where there is a hit."""
    objs = G.SCENES[scene]()
    rays, spans = scene_rays(scene)
    reading = G.Reading(objs, G.HEURISTICS[heur])
    t, obj = reading.intersect(rays.o, rays.d)
    for family, sl in spans.items():
        G.check_family_edges(scene, family, reading, G.Rays(rays.o[sl], rays.d[sl], rays.aim[sl]), t[sl], obj[sl],
                             reading.stats["tie"][sl], reading.stats["flat_entered"])
    osc = _oracle.OracleScene(objs, G.T0, G.T1, G.HEURISTICS[heur], HDRI)
    rt, robj = osc.intersect_batch(rays.o, rays.d, G.T0, G.T1, traversal=0)  # orc_bvh_intersect, as intersect_many
    assert np.array_equal(obj, robj)
    assert np.array_equal(bits(t), bits(rt))
    prod = rayrs_amd.Scene(objs, G.T0, G.T1, G.HEURISTICS[heur], HDRI, device=-1)
    info = prod.info()
    if scene.startswith("mesh") or scene == "floor_spheres":
        assert info["hot_count"] >= 1 and info["compact"] == (1 if scene.startswith("mesh") else 0)
    osc.use_product_walk(prod)
    wt, wobj = osc._with_margin(2, lambda: osc.intersect_batch(rays.o, rays.d, G.T0, G.T1, traversal=2))
    assert np.array_equal(obj, wobj)
    assert np.array_equal(bits(t), bits(wt))
    assert (obj >= 0).sum() > 0
