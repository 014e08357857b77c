"""The radiance queries with a mesh-light group chosen by a light tree (include/rayrs_hip.h LIGHT TREE) on the GPU, bit for bit and
count for count against the plain-Python reading of the operation (tests/_tree.py), on both walks, in the three forms.  Every
answer of the reading on these scenes is finite, so the comparison is of bits throughout.

The scenes: tests/_mesh.py's room (f64 records; its group is a dozen triangles of two emissions: two quads and an octahedron) with
K = 0, 2 and 8 lamps, without and with the sky, and with groups of its first 1, 2 and 3 triangles; and its small version with the
one quad, which is of the local-pool route's size.  130 rays or points are two full waves and a partial one; five samples in
chunks of two span three chunks."""
import functools
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import _mesh
import _oracle
import _tree
import rayrs_amd
from rayrs_amd import SKY, procedural, scenes
from test_gpu_mesh_lights import mesh1_objects
from test_gpu_radiance import primary_rays

pytestmark = pytest.mark.gpu

HDRI = procedural.make_studio_hdri(9, 5)
Z_NEAR, Z_FAR = 1e-6, 1e6
S = 5
SEED = 0x5EED
W, H = 13, 10   # 130 rays, 130 points


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def family(name, n_group=None):
    return _family(name, n_group)   # (one cache key however it is called: a family's tally is its own)


@functools.lru_cache(maxsize=None)
def _family(name, n_group):
    if name == "mesh1":   # tests/test_gpu_mesh_lights.py's: compact records, a hot group, a fast walk of its own, a deeper tree
        cam_args, objs, heur, tris = mesh1_objects()
        lists = {"none": (), "lamp": tuple(rayrs_amd.emitters(objs))}
        assert len(lists["lamp"]) == 1 and len(tris) >= 20 and n_group is None
    else:
        cam_args, objs, heur, names = _mesh.mesh_room(small=name == "small")
        lamp, rect, dark = names["sphere_lamp"], names["rect_lamp"], names["dark_sphere"]
        lists = {"none": (), "two": (lamp, rect), "eight": (lamp, rect, dark, lamp, rect, rect, dark, lamp)}
        tris = names["group"] if n_group is None else names["group"][:n_group]
    scene = rayrs_amd.Scene(objs, Z_NEAR, Z_FAR, heur, HDRI, device=0)
    mesh = scene.mesh_lights(tris, tree=True)
    o, d = primary_rays(cam_args, W, H)
    fast_osc = _oracle.OracleScene(objs, Z_NEAR, Z_FAR, heur, HDRI).use_product_walk(scene, fast=True)
    readings = {False: _tree.Reading(objs, Z_NEAR, Z_FAR, heur, HDRI, tris),
                True: _tree.Reading(objs, Z_NEAR, Z_FAR, heur, HDRI, tris, osc=fast_osc, traversal=2)}
    p = np.array([(xi, 0.0, zi) for zi in np.linspace(-3.5, 3.5, H) for xi in np.linspace(-3.5, 3.5, W)])
    nrm = np.tile((0.0, 1.0, 0.0), (len(p), 1))
    assert len(o) == len(p) == 130 and len(mesh) == len(tris)
    for x in (o, d, p, nrm):
        x.setflags(write=False)
    return SimpleNamespace(cam_args=scenes.camera_for_resolution(cam_args, 20, 12), o=o, d=d, p=p, nrm=nrm, scene=scene, mesh=mesh,
                           tris=tris, objs=objs, heur=heur, readings=readings, lists=lists, info=scene.info(), tally=_mesh.new_tally())


def lights_of(f, which, sky):
    return list(f.lists[which]) + ([SKY] if sky else [])


def expected(name, which, sky, what, fast=False, samples=S, max_bounces=50, n_group=None):
    """The reading's paths of the family's rays ("radiance"), points ("irradiance") or pixels ("image"): (values, queries), made
    once.  The default walk's paths at the default sizes feed the family's tally."""
    return _expected(name, which, sky, what, fast, samples, max_bounces, n_group)


@functools.lru_cache(maxsize=None)
def _expected(name, which, sky, what, fast, samples, max_bounces, n_group):
    f = family(name, n_group)
    R = f.readings[fast]
    tally = f.tally if not fast and samples == S and max_bounces == 50 else None
    lights = lights_of(f, which, sky)
    if what == "radiance":
        return _tree.radiance_paths(R, f.o, f.d, samples, max_bounces, SEED, lights, tally=tally)
    if what == "irradiance":
        return _tree.irradiance_paths(R, f.p, f.nrm, samples, 1e-4, max_bounces, SEED, lights, tally=tally)
    return _tree.image_paths(R, _oracle.OracleCamera(*f.cam_args), samples, max_bounces, SEED, lights, tally=tally)


def check(got, values, queries, chunk, what):
    rad, cnt = got
    want_rad, want_cnt = _tree.answers(values, queries, chunk)
    assert np.isfinite(want_rad).all(), what
    assert rad.dtype == np.float64 and cnt.dtype == np.uint32 and rad.shape == want_rad.shape and cnt.shape == want_cnt.shape, what
    bad = np.flatnonzero(cnt != want_cnt)
    assert len(bad) == 0, (what, "queries", len(bad), [(int(i), int(cnt[i]), int(want_cnt[i])) for i in bad[:5]])
    bad = np.flatnonzero((bits(rad) != bits(want_rad)).any(axis=1))
    assert len(bad) == 0, (what, "radiance", len(bad), [(int(i), rad[i].tolist(), want_rad[i].tolist()) for i in bad[:3]])


CASES = [("room", "none", False, None), ("room", "none", True, None), ("room", "two", False, None), ("room", "two", True, None),
         ("room", "eight", False, None), ("room", "eight", True, None), ("small", "two", True, None), ("small", "none", False, None),
         ("room", "two", True, 1), ("room", "two", False, 2), ("room", "none", True, 3), ("mesh1", "lamp", True, None),
         ("mesh1", "none", False, None)]


# ------------------------------------------------------------------------------------------------------ parity

@pytest.mark.parametrize("name,which,sky,n_group", CASES)
def test_tree_radiance_and_queries_are_the_readings(name, which, sky, n_group):
    f = family(name, n_group)
    assert f.mesh.tree and len(f.mesh) == (n_group or {"small": 2, "room": 12}.get(name, len(f.tris)))
    assert (f.info["local_pool"] == 1) == (name == "small") and (f.info["compact"] == 1) == (name == "mesh1"), f.info
    lights = lights_of(f, which, sky)
    for fast in (False, True):
        values, queries = expected(name, which, sky, "radiance", fast, n_group=n_group)
        check(f.scene.radiance(f.o, f.d, samples=S, seed=SEED, sample_chunk=2, fast_traversal=fast, queries=True, lights=lights, direct=True,
                               mesh=f.mesh), values, queries, 2, (name, which, sky, n_group, fast))


@pytest.mark.parametrize("name,which,sky,n_group", CASES)
def test_tree_irradiance_at_points_is_the_readings(name, which, sky, n_group):
    f = family(name, n_group)
    lights = lights_of(f, which, sky)
    for fast in (False, True):
        values, queries = expected(name, which, sky, "irradiance", fast, n_group=n_group)
        check(f.scene.irradiance(f.p, f.nrm, samples=S, bias=1e-4, seed=SEED, sample_chunk=2, fast_traversal=fast, queries=True, lights=lights,
                                 direct=True, mesh=f.mesh), values, queries, 2, (name, which, sky, n_group, fast))


@pytest.mark.parametrize("name,which,sky", [("room", "eight", True), ("room", "none", False), ("small", "two", True), ("mesh1", "lamp", True)])
def test_render_with_a_tree_is_the_readings(name, which, sky):
    """Both values of fast_traversal; the image form takes the walk a render with its settings takes (on the local-pool-sized
    small room the default walk whatever is asked)."""
    f = family(name)
    cam = rayrs_amd.Camera(*f.cam_args)
    assert (cam.x_pixels(), cam.y_pixels()) == (20, 12)
    for fast in (False, True):
        values, queries = expected(name, which, sky, "image", fast and f.info["local_pool"] == 0, samples=3)
        img, cnt = rayrs_amd.render_lit(f.scene, cam, 3, lights_of(f, which, sky), seed=SEED, sample_chunk=2, fast_traversal=fast, queries=True,
                                        direct=True, mesh=f.mesh)
        assert img.shape == (12, 20, 3) and cnt.shape == (12, 20)
        check((img.reshape(-1, 3), cnt.reshape(-1)), values, queries, 2, (name, which, sky, "image", fast))


@pytest.mark.parametrize("max_bounces", [0, 1])
def test_the_bounce_bound(max_bounces):
    """0 is +0 and no query, no shadow query either; with 1 the shadow sample of the one bounce is traced and credited."""
    f = family("room")
    lights = lights_of(f, "two", True)
    if max_bounces == 0:
        for call, a, b, kw in ((f.scene.radiance, f.o, f.d, {}), (f.scene.irradiance, f.p, f.nrm, dict(bias=1e-4))):
            rad, cnt = call(a, b, samples=3, max_bounces=0, queries=True, lights=lights, direct=True, mesh=f.mesh, **kw)
            assert rad.shape == (len(a), 3) and not bits(rad).any() and not cnt.any()
        return
    for what, call, a, b, kw in (("radiance", f.scene.radiance, f.o, f.d, {}), ("irradiance", f.scene.irradiance, f.p, f.nrm, dict(bias=1e-4))):
        values, queries = expected("room", "two", True, what, max_bounces=1)
        check(call(a, b, samples=S, seed=SEED, max_bounces=1, sample_chunk=2, queries=True, lights=lights, direct=True, mesh=f.mesh, **kw),
              values, queries, 2, (what, "one bounce"))
        assert queries.max() == (2 if what == "radiance" else 3)


def test_a_slice_with_its_index_base_is_the_slice_of_the_whole():
    f = family("room")
    kw = dict(samples=S, seed=SEED, sample_chunk=2, queries=True, lights=lights_of(f, "two", True), direct=True, mesh=f.mesh)
    rad, cnt = f.scene.radiance(f.o, f.d, **kw)
    n = len(f.o)
    for a, b in ((0, 1), (1, 70), (70, 129), (129, n)):
        r, c = f.scene.radiance(f.o[a:b], f.d[a:b], index_base=a, **kw)
        assert np.array_equal(c, cnt[a:b]) and np.array_equal(bits(r), bits(rad[a:b])), (a, b)
    irr, icnt = f.scene.irradiance(f.p, f.nrm, bias=1e-4, **kw)
    r, c = f.scene.irradiance(f.p[7:120], f.nrm[7:120], bias=1e-4, index_base=7, **kw)
    assert np.array_equal(c, icnt[7:120]) and np.array_equal(bits(r), bits(irr[7:120]))
    for call in (f.scene.radiance, f.scene.irradiance):
        r0, c0 = call(np.zeros((0, 3)), np.zeros((0, 3)), samples=3, queries=True, lights=[], direct=True, mesh=f.mesh)
        assert r0.shape == (0, 3) and c0.shape == (0,)


def test_device_tensors_on_a_stream_give_the_host_paths_bits():
    """tests/_tree_torch_child.py, in a process of its own (torch has to be imported before the library is loaded)."""
    pytest.importorskip("torch")
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_tree_torch_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "device path ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


# ------------------------------------------------------------------------------------------------------ not vacuous

def test_the_comparison_is_not_vacuous():
    """The tree's answers differ from the area group's on the same scene, and -- from the reading alone, over the default walk's
    paths of the room's cases above -- a meaningful share of the paths' diffuse bounces credits a tree-drawn shadow sample, listed
    triangles are met with the tree's weight, and the other branches are taken."""
    f = family("room")
    area = f.scene.mesh_lights(f.tris)
    for lights in ([], lights_of(f, "two", True)):
        kw = dict(samples=S, seed=SEED, sample_chunk=2, queries=True, lights=lights, direct=True)
        t, a = f.scene.radiance(f.o, f.d, mesh=f.mesh, **kw), f.scene.radiance(f.o, f.d, mesh=area, **kw)
        assert (bits(t[0]) != bits(a[0])).any(axis=1).sum() >= 30, lights
        t, a = f.scene.irradiance(f.p, f.nrm, bias=1e-4, mesh=f.mesh, **kw), f.scene.irradiance(f.p, f.nrm, bias=1e-4, mesh=area, **kw)
        assert (bits(t[0]) != bits(a[0])).any(axis=1).sum() >= 30, lights
    area.close()
    for name, which, sky, n_group in CASES:
        if name == "room" and n_group is None:
            expected(name, which, sky, "radiance"), expected(name, which, sky, "irradiance")
    t = f.tally
    print(t)
    drawn = sum(t[k] for k in t if k.startswith("group_"))
    assert drawn >= 1000 and t["group_credited"] >= drawn // 4, t    # of the draws of the group, a quarter at least earn
    assert t["group_skipped_ndl"] >= 10 and t["group_blocked_unlisted"] + t["group_blocked_listed"] >= 10, t
    assert t["met_listed_weighted"] >= 10 and t["met_listed_unweighted"] >= 1, t
    assert t["lamp_credited"] >= 100 and t["sky_credited"] >= 100, t


# ------------------------------------------------------------------------------------------------------ non-finite input

def test_points_and_normals_with_nan_and_infinite_components_end_and_the_finite_ones_are_the_readings():
    """A third of the points has a NaN or an infinite component in the position or the normal: the descent ends for every f64
    point, so the call does, and a finite point's answer is the reading's of that point at its index."""
    f = family("room")
    p, nrm = f.p.copy(), f.nrm.copy()
    bad = (np.nan, np.inf, -np.inf)
    for i in range(0, len(p), 3):
        (p if (i // 3) % 2 else nrm)[i, (i // 3) % 3] = bad[(i // 9) % 3]
    finite = np.isfinite(p).all(axis=1) & np.isfinite(nrm).all(axis=1)
    assert 40 <= (~finite).sum() <= 50
    lights = lights_of(f, "two", True)
    some = np.flatnonzero(finite)[::4]
    for fast in (False, True):
        rad, cnt = f.scene.irradiance(p, nrm, samples=S, bias=1e-4, seed=SEED, sample_chunk=2, fast_traversal=fast, queries=True, lights=lights,
                                      direct=True, mesh=f.mesh)
        assert rad.shape == (len(p), 3) and np.isfinite(rad[finite]).all()
        for i in some:
            values, queries = _tree.irradiance_paths(f.readings[fast], p[i:i + 1], nrm[i:i + 1], S, 1e-4, 50, SEED, lights, index_base=int(i))
            check((rad[i:i + 1], cnt[i:i + 1]), values, queries, 2, ("point", int(i), fast))
    o = f.o.copy()
    o[::3, 1] = np.nan
    rad, cnt = f.scene.radiance(o, f.d, samples=S, seed=SEED, sample_chunk=2, queries=True, lights=lights, direct=True, mesh=f.mesh)
    whole = f.scene.radiance(f.o, f.d, samples=S, seed=SEED, sample_chunk=2, queries=True, lights=lights, direct=True, mesh=f.mesh)
    keep = np.ones(len(o), dtype=bool)
    keep[::3] = False
    assert np.array_equal(bits(rad[keep]), bits(whole[0][keep])) and np.array_equal(cnt[keep], whole[1][keep])


# ------------------------------------------------------------------------------------------------------ handles and neighbours

def test_a_tree_handle_and_an_area_handle_each_give_their_own_bits_and_closing_one_leaves_the_other():
    f = family("room")
    area, other = f.scene.mesh_lights(f.tris), f.scene.mesh_lights(f.tris[::2], tree=True)
    kw = dict(samples=S, seed=SEED, sample_chunk=2, queries=True, lights=lights_of(f, "two", False), direct=True)
    t0, a0, o0 = (f.scene.radiance(f.o, f.d, mesh=m, **kw) for m in (f.mesh, area, other))
    assert (bits(t0[0]) != bits(a0[0])).any() and (bits(t0[0]) != bits(o0[0])).any()
    for _ in range(2):
        for m, want in ((area, a0), (f.mesh, t0), (other, o0)):
            got = f.scene.radiance(f.o, f.d, mesh=m, **kw)
            assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1])
    area.close()
    got = f.scene.radiance(f.o, f.d, mesh=f.mesh, **kw)
    assert np.array_equal(bits(got[0]), bits(t0[0])) and np.array_equal(got[1], t0[1])
    other.close()
    area = f.scene.mesh_lights(f.tris)
    got = f.scene.radiance(f.o, f.d, mesh=area, **kw)
    assert np.array_equal(bits(got[0]), bits(a0[0])) and np.array_equal(got[1], a0[1])
    area.close()
    with pytest.raises(ValueError):
        f.scene.radiance(f.o, f.d, mesh=other, **kw)
    with pytest.raises(rayrs_amd._ffi.RayrsError) as e:   # a handle of another scene is refused
        f.scene.radiance(f.o, f.d, mesh=family("small").mesh, **kw)
    assert e.value.status == -1
    empty = f.scene.mesh_lights([], tree=True)              # an empty tree group: DIRECT LIGHTING's bits
    want = f.scene.radiance(f.o, f.d, **kw)
    got = f.scene.radiance(f.o, f.d, mesh=empty, **kw)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1])
    empty.close()
    cam = rayrs_amd.Camera(*f.cam_args)
    for make in (lambda: rayrs_amd.Film(f.scene, cam, lights=[], direct=True, mesh=f.mesh),
                 lambda: rayrs_amd.Bake(f.scene, f.p, f.nrm, lights=[], direct=True, mesh=f.mesh)):
        with pytest.raises(rayrs_amd._ffi.RayrsError) as e:   # films and bakes do not take a tree
            make()
        assert e.value.status == -5


def test_a_render_and_a_direct_call_are_the_same_before_and_after_a_batch_of_tree_calls():
    f = family("room")
    cam = rayrs_amd.Camera(*f.cam_args)
    lamps = list(f.lists["two"])
    before, st0 = rayrs_amd.render(f.scene, cam, 4, out_f64=True)
    direct0 = f.scene.radiance(f.o, f.d, samples=S, lights=lamps, direct=True)
    for fast in (False, True):
        f.scene.radiance(f.o, f.d, samples=S, sample_chunk=2, fast_traversal=fast, lights=lamps + [SKY], direct=True, mesh=f.mesh)
        f.scene.irradiance(f.p, f.nrm, samples=8, bias=1e-4, fast_traversal=fast, lights=[], direct=True, mesh=f.mesh)
        rayrs_amd.render_lit(f.scene, cam, 2, [SKY], fast_traversal=fast, direct=True, mesh=f.mesh)
    after, st1 = rayrs_amd.render(f.scene, cam, 4, out_f64=True)
    direct1 = f.scene.radiance(f.o, f.d, samples=S, lights=lamps, direct=True)
    assert before.tobytes() == after.tobytes() and direct0.tobytes() == direct1.tobytes()
    assert st0["rays"] == st1["rays"] and st0["paths"] == st1["paths"]
