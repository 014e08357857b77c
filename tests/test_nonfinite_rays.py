"""Non-finite and far-scaled rays, and open z windows, without a GPU (include/rayrs_hip.h RAY QUERIES: "any f64 is a legal
component"; rayrs_scene_new: z_near >= 0 and any z_far > z_near).  On the rays of tests/_nonfinite_rays.py, under the windows
(1e-6, 1e6), (0, +inf) and (2^-1060, 2^1020), bit for bit and with no ray left out:

  * the second reading (tests/_geometry_reading.py) against the oracle's recursion and against the oracle's walk of the
    product's own records, hot group included;
  * each primitive test and the box test of the primitive's own box against the oracle's;
  * the classes' conditions (_nonfinite_rays.check_classes), from the reading alone;
  * the oracle's walk of the product's fast tree runs on every class: what the fast walk of the kernels is held to;
  * _ao.directions on a table of edge normals against the oracle's Lambertian scatter direction, NaN places included.

tests/test_gpu_nonfinite_rays.py holds the kernels to the same answers."""
import functools
import itertools

import numpy as np
import pytest

import _ao
import _geometry_reading as G
import _nonfinite_rays as N
import _oracle
import rayrs_amd
from _nonfinite import assert_same_frame_nan_aware
from rayrs_amd import procedural
from rayrs_amd.api import Material
from test_second_reading_of_geometry_rs import _orc

HDRI = procedural.make_hdri(8, 4)
CASES = [(s, h, w) for s, h in N.BUILDERS for w in N.WINDOWS]
IDS = [f"{s}-{h}-{w}" for s, h, w in CASES]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def rays_of(scene):
    rays, spans = N.nonfinite_rays(scene)
    rays.o.setflags(write=False), rays.d.setflags(write=False)
    return rays, spans


@functools.lru_cache(maxsize=None)
def reader(scene, heur):
    return G.Reading(G.SCENES[scene](), G.HEURISTICS[heur])


@functools.lru_cache(maxsize=None)
def reading(scene, heur, window):
    """(t, object) of the scene's rays under the window, as the second reading has them."""
    rays, _ = rays_of(scene)
    t, obj = reader(scene, heur).intersect(rays.o, rays.d, *N.WINDOWS[window])
    t.setflags(write=False), obj.setflags(write=False)
    return t, obj


@functools.lru_cache(maxsize=None)
def host_product(scene, heur, window):
    return rayrs_amd.Scene(G.SCENES[scene](), *N.WINDOWS[window], G.HEURISTICS[heur], HDRI, device=-1)


def hot_objects(scene, heur, window):
    """The objects of the product's hot group, None where the scene has none."""
    prod = host_product(scene, heur, window)
    info = prod.info()
    if not info["hot_count"]:
        return None
    pp = prod.export_bvh()[2]
    return [int(pp[info["hot_first"] + k]) for k in range(info["hot_count"])]


def oracle_scene(scene, heur, window):
    return _oracle.OracleScene(G.SCENES[scene](), *N.WINDOWS[window], G.HEURISTICS[heur], HDRI)


@functools.lru_cache(maxsize=None)
def fast_walk(scene, heur, window):
    """The oracle's walk of the product's fast tree with the kernel's cull margin: what rayrs_test_trace (exact = 0) and
    fast_traversal = 1 are held to."""
    rays, _ = rays_of(scene)
    tmin, tmax = N.WINDOWS[window]
    osc = oracle_scene(scene, heur, window).use_product_walk(host_product(scene, heur, window), fast=True)
    t, obj = osc._with_margin(2, lambda: osc.intersect_batch(rays.o, rays.d, tmin, tmax, traversal=2, nthreads=16))
    t.setflags(write=False), obj.setflags(write=False)
    return t, obj


@functools.lru_cache(maxsize=None)
def fast_tree(scene, heur, window):
    """The oracle's walk of the product's fast tree with nothing culled (test_gpu_queries.fast_tree_reading's recipe): what
    the any-hit queries on that tree are held to."""
    rays, _ = rays_of(scene)
    tmin, tmax = N.WINDOWS[window]
    osc = oracle_scene(scene, heur, window).use_walk_tree(host_product(scene, heur, window))
    try:
        _oracle.set_cull_margin(float("inf"))
        t, obj = osc.intersect_batch(rays.o, rays.d, tmin, tmax, traversal=2, nthreads=16)
    finally:
        _oracle.set_cull_margin(2.0 ** -10)
    t.setflags(write=False), obj.setflags(write=False)
    return t, obj


def assert_same(got, want, what):
    """The object everywhere, the bits of t where there is a hit."""
    (t, obj), (rt, robj) = got, want
    bad = np.flatnonzero((obj != robj) | ((robj >= 0) & (bits(t) != bits(rt))))
    assert len(bad) == 0, (what, len(bad), [(int(i), int(obj[i]), int(robj[i]), float(t[i]), float(rt[i])) for i in bad[:5]])


# ------------------------------------------------------------------------------------------------------ the layout

def test_every_class_lies_in_whole_workgroups_and_between_ordinary_rays():
    for scene in N.SCENES:
        rays, spans = rays_of(scene)
        n = len(rays.o)
        assert n % 256 != 0 and 20000 <= n <= 30000
        seen = np.zeros(n, dtype=int)
        for name in N.CLASSES:
            run, mixed = spans[name]
            assert run.start % 256 == 0 and run.stop - run.start == 256 and mixed.step == 2
            seen[run] += 1
            seen[mixed] += 1
            between = np.arange(n)[mixed] + 1
            assert spans["ordinary"][0][between].all() and len(between) == 256
        assert (seen + spans["ordinary"][0] == 1).all()
        ordinary = spans["ordinary"][0]
        assert np.isfinite(rays.o[ordinary]).all() and np.isfinite(rays.d[ordinary]).all()
        # the existing families are as they were: these rays are no case of theirs
        assert not any("nan" in f or "scale" in f for f in G.FAMILIES)
    cls = {c: N.class_index(rays_of("soup")[1], c, n) for c in N.CLASSES}
    rays = rays_of("soup")[0]
    assert np.isnan(rays.d[cls["d_nan_all"]]).all() and np.isnan(rays.o[cls["o_nan_all"]]).all()
    assert (np.isnan(rays.d[cls["d_nan_one"]]).sum(axis=1) == 1).all() and (np.isnan(rays.o[cls["o_nan_one"]]).sum(axis=1) == 1).all()
    assert (np.isposinf(rays.d[cls["d_pinf_one"]]).sum(axis=1) == 1).all() and (np.isneginf(rays.d[cls["d_ninf_one"]]).sum(axis=1) == 1).all()
    assert (np.isposinf(rays.o[cls["o_pinf_one"]]).sum(axis=1) == 1).all() and (np.isneginf(rays.o[cls["o_ninf_one"]]).sum(axis=1) == 1).all()
    assert (np.isposinf(rays.o[cls["o_pinf_d_pinf"]]) == np.isposinf(rays.d[cls["o_pinf_d_pinf"]])).all()
    assert (np.isposinf(rays.o[cls["o_pinf_d_ninf"]]) == np.isneginf(rays.d[cls["o_pinf_d_ninf"]])).all()
    for name in ("d_pzero_inside", "d_nzero_inside"):
        assert (rays.d[cls[name]] == 0.0).all() and np.signbit(rays.d[cls[name]]).any() and not np.signbit(rays.d[cls[name]]).all()
    assert ((np.abs(rays.d[cls["d_denormal_one"]]) == 5e-324).sum(axis=1) == 1).all()
    mags = {k: np.abs(rays.d[cls[f"scale_2^{k}"]]).max(axis=1) for k in N.SCALES}
    assert all((m > 2.0 ** (k - 8)).all() and (m < 2.0 ** (k + 8)).all() for k, m in mags.items())


# ------------------------------------------------------------------------------------------------------ whole queries

@pytest.mark.parametrize("scene,heur,window", CASES, ids=IDS)
def test_whole_queries_are_the_oracles_under_every_window(scene, heur, window):
    """The reading's recursion, the oracle's recursion and the oracle's walk of the product's own records (the gate tree, the
    hot group beside it where there is one) agree on the object everywhere and on the bits of t where there is a hit; the
    classes show what they are made for."""
    rays, spans = rays_of(scene)
    tmin, tmax = N.WINDOWS[window]
    t, obj = reading(scene, heur, window)
    hot = hot_objects(scene, heur, window)
    assert (hot is not None) == (scene in N.HOT_SCENES)
    hits = N.check_classes(scene, window, reader(scene, heur), rays, spans, t, obj, hot)
    print(scene, heur, window, "hits per class of", 2 * N.RUN, hits)
    osc = oracle_scene(scene, heur, window)
    rt, robj = osc.intersect_batch(rays.o, rays.d, tmin, tmax, traversal=0)
    assert_same((rt, robj), (t, obj), "the oracle's recursion")
    assert np.array_equal(bits(t), bits(rt))
    osc.use_product_walk(host_product(scene, heur, window))
    wt, wobj = osc._with_margin(2, lambda: osc.intersect_batch(rays.o, rays.d, tmin, tmax, traversal=2))
    assert_same((wt, wobj), (t, obj), "the oracle's walk of the product's records")
    assert np.array_equal(bits(t), bits(wt))
    assert (obj >= 0).sum() > 0


@pytest.mark.parametrize("scene,heur,window", CASES, ids=IDS)
def test_the_oracles_walk_of_the_fast_tree_runs_on_every_class(scene, heur, window):
    """The fast walk promises nothing against the reading: the kernels' fast walk is held to this walk.  It answers every ray;
    a reported hit is one the reading's primitive test accepts within the window, no nearer than the reading's closest hit."""
    rays, spans = rays_of(scene)
    tmin, tmax = N.WINDOWS[window]
    ft, fobj = fast_walk(scene, heur, window)
    t, obj = reading(scene, heur, window)
    n = len(rays.o)
    assert ft.shape == (n,) and not np.isnan(ft).any() and (fobj >= -1).all() and (fobj < len(reader(scene, heur).prims)).all()
    hit = fobj >= 0
    with np.errstate(all="ignore"):
        some, pt, _ = reader(scene, heur).prims.intersect(np.where(hit, fobj, 0), G.vec(rays.o), G.vec(rays.d))
    assert (some & (bits(pt) == bits(ft)) & (pt > tmin) & (pt < tmax))[hit].all()
    assert (obj[hit] >= 0).all() and (ft[hit] >= t[hit]).all()
    # the tree with nothing culled finds a hit exactly where the reading does
    nt, nobj = fast_tree(scene, heur, window)
    assert np.array_equal(nobj >= 0, obj >= 0)


# ------------------------------------------------------------------------------------------------------ per primitive

def oracle_primitive(prims, aim, o, d, tmin, tmax):
    """test_second_reading_of_geometry_rs.oracle_primitive with the window passed to the box test."""
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
        boxed[i] = aab(pb + 48 * k, oi, di, tmin, tmax) != 0
    return some, t, boxed


@pytest.mark.parametrize("scene", N.SCENES)
def test_each_primitive_test_is_the_oracles(scene):
    """Sphere / Plane / Triangle::intersect (the hit flag; where there is one, t bit for bit or NaN on both sides) for every ray
    against the object it is put to, and the box test of the object's own box under each window."""
    rays, spans = rays_of(scene)
    o, d = np.ascontiguousarray(rays.o), np.ascontiguousarray(rays.d)
    prims = reader(scene, "sah1000").prims
    with np.errstate(all="ignore"):
        some, t, _ = prims.intersect(rays.aim, G.vec(o), G.vec(d))
    for window, (tmin, tmax) in N.WINDOWS.items():
        with np.errstate(all="ignore"):
            boxed = G.aabb_intersect(tuple(prims.box[rays.aim].T), G.vec(o), G.vec(d), tmin, tmax)
        osome, ot, oboxed = oracle_primitive(prims, rays.aim, o, d, tmin, tmax)
        assert np.array_equal(some, osome), window
        assert_same_frame_nan_aware(t[some], ot[some], f"{scene} t")
        assert np.array_equal(boxed, oboxed), window
        assert some.sum() > 0 and boxed.sum() > 0
    nan_t = some & np.isnan(t)
    print(scene, "Some(NaN)", int(nan_t.sum()))
    if (prims.kind == 2).any():   # Triangle::intersect's Some(NaN): a hit whose t the leaf's window then refuses
        assert nan_t.sum() >= 100, int(nan_t.sum())


# ------------------------------------------------------------------------------------------------------ edge normals

EDGE_VALUES = (0.0, -0.0, 1.0, -1.0, 2.0, 5e-324, 1e-310, 1e-160, 1e-155, 1e-100, 1e100, 1e154, 1.4e154, 1e200, 1.7e308,
               float("inf"), float("-inf"), float("nan"))
TIES = ((3.0, -3.0, 1.0), (-0.5, 0.5, 2.0), (0.25, 0.25, -1.0), (1e-200, -1e-200, 1.0), (1e250, 1e250, 1e-250), (-7.0, -7.0, 0.0))


@functools.lru_cache(maxsize=None)
def edge_normals():
    """Every triple of EDGE_VALUES, and ties |x| == |y| (the basis takes its first vector from the larger of the two)."""
    n = np.array(list(itertools.product(EDGE_VALUES, repeat=3)) + list(TIES), dtype=np.float64)
    n.setflags(write=False)
    return n


def edge_keys(n):
    return [_ao.path_key(0xED6E, i, i % 7) for i in range(n)]


def test_the_readings_directions_are_the_oracles_on_edge_normals():
    normals = edge_normals()
    assert len(normals) == 5838
    keys = edge_keys(len(normals))
    got = _ao.directions(normals, keys)
    scattered, _, want, draws = _oracle.material_evaluate(Material.LambertianDiffuse((0.5, 0.5, 0.5)), normals, normals, keys)
    assert scattered.all() and (draws == 2).all()
    assert_same_frame_nan_aware(got, want, "edge normals")
    finite = np.isfinite(got).all(axis=1)
    print("finite directions", int(finite.sum()), "of", len(normals))
    assert finite.sum() >= 1000 and (~finite).sum() >= 1000


# ------------------------------------------------------------------------------------------------------ the stack

def every_slot_walk(ref, root):
    """device_path.h trav_interior_step for a ray that enters all four slots of every record -- an all-NaN ray: its entry
    parameters are all t0, so it walks in slot order, the unused slots included (their reference reads as a leaf group).
    Returns (the most entries it has waiting, its steps)."""
    stack, cur, most, steps = [], int(root), 0, 0
    while cur is not None:
        steps += 1
        if cur >> 30 == 0:
            r = [int(x) for x in ref[cur & 0x3fffffff]]
            cur = r[0]
            stack.extend(reversed(r[1:]))
            most = max(most, len(stack))
        else:
            cur = stack.pop() if stack else None
    return most, steps


def row_of_spheres(n):
    from rayrs_amd.api import Emission, Object
    return [Object.sphere(0.4, (3.0 * i, 0.0, 0.0), Material.NoReflect(), Emission.Dark()) for i in range(n)]


def test_a_lanes_stack_holds_the_walk_of_a_ray_that_enters_every_slot():
    """The slab test ignores a NaN slab, so a ray with a NaN direction or origin enters every box -- the inverted box of an
    unused slot too -- and on a record with fewer than four used slots has more slots waiting than any finite ray.  A lane's
    stack (rayrs_lab_stack_need) holds the depth a scene reports for a tree and that walk, on every tree, also on the small
    trees (one record with two or three groups: the reference's sphere scenes) where the walk is the larger need."""
    from rayrs_amd import scenes
    makers = {s: G.SCENES[s] for s in G.SCENES}
    makers.update(material_test=lambda: scenes.material_test()[1], metallic=lambda: scenes.cook_torrance_spheres_metallic()[1],
                  single_sphere=lambda: scenes.diffuse_single_sphere()[1])
    makers.update({f"row{n}": (lambda n=n: row_of_spheres(n)) for n in (3, 5, 6, 7, 9, 11, 13)})
    underfilled = 0
    for name, make in makers.items():
        for heur in ("sah1000", "midpoint"):
            prod = rayrs_amd.Scene(make(), G.T0, G.T1, G.HEURISTICS[heur], HDRI, device=-1)
            info = prod.info()
            trees = [(prod.export_wide, "wide_", 0), (prod.export_gate_tree, "gate_", 1)] + \
                    ([(prod.export_hot_tree, "hot_", 2)] if info["hot_count"] else [])
            if not info["hot_count"]:
                assert prod._L.rayrs_lab_stack_need(prod._h, 2) == -1
            for export, pre, which in trees:
                ref = export()[1]
                if len(ref) == 0:
                    continue
                root = info[pre + "root_ref"]
                most, steps = every_slot_walk(ref, root)
                need = prod.lab_stack_need(which)
                assert need == max(most, info[pre + "depth"]), (name, heur, pre, most, info[pre + "depth"], need)
                assert steps == 1 + 4 * len(ref)      # every slot of every record once, and the root
                underfilled += int(most > info[pre + "depth"])
    assert underfilled >= 5   # trees on which this walk needs more than the reported depth
