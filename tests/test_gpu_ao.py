"""Ambient occlusion (include/rayrs_hip.h AMBIENT OCCLUSION) on the GPU, count for count against the plain-Python reading of
the operation (tests/_ao.py) whose verdicts come from the second reading of geometry.rs and bvh.rs (tests/_geometry_reading.py),
with G.T0, G.T1 as z_near, z_far.  The points are hit positions of the scenes' seeded ray families -- every k-th hit, 3,000 of
them -- with the normal of tests/_features.py's object table turned against the ray; S = 5 makes 15,000 items, no multiple of 64.

The kernel hands a point's samples to whichever lanes are idle, so besides the parity there are the shapes where that schedule
can go wrong, every refill setting, batches cut in pieces and across launches, device tensors on a stream, the image form
against the oracle alone, a render before and after, and the command line."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import _ao
import _features as F
import _geometry_reading as G
import _oracle
import rayrs_amd
from rayrs_amd import _ffi, io, procedural, scenes
from test_gpu_geometry_reading import HDRI, bits, device_scene, reading, scene_rays

pytestmark = pytest.mark.gpu

CLI = os.path.join(os.path.dirname(os.path.abspath(rayrs_amd.__file__)), "rayrs")
S = 5
SEED = 0x5EED
N_POINTS = 3000
PARITY = [(s, "sah1000") for s in ("floor_spheres", "mesh1280_light", "soup", "ties")] + [("soup", "midpoint")]
IDS = [f"{s}-{h}" for s, h in PARITY]
CONDITION = ("floor_spheres", "mesh1280_light", "soup")   # (ties is exempt: 9 occluded samples at a small radius)


def normals_at(objs, obj, p):
    """object_table(objs)[object] at the positions p."""
    out = np.zeros((len(obj), 3))
    with np.errstate(all="ignore"):
        table = F.object_table(objs)
        for k in np.unique(obj):
            m = obj == k
            nx, ny, nz = table[int(k)][0](G.take(G.vec(p), m))
            out[m, 0], out[m, 1], out[m, 2] = nx, ny, nz
    return out


@functools.lru_cache(maxsize=None)
def ao_points(scene, heur):
    """(points, normals, extent): the hit positions of every k-th hit of the scene's reading, the normals turned against the
    ray, points whose normal is not finite dropped; extent = the diagonal of the points' bounding box."""
    rays, _ = scene_rays(scene)
    rt, robj = reading(scene, heur)
    hit = np.flatnonzero(robj >= 0)
    sel = hit[::max(1, len(hit) // N_POINTS)][:N_POINTS]
    p = np.stack(G.point(G.vec(rays.o[sel]), G.vec(rays.d[sel]), rt[sel]), axis=1)
    n = _ao.turned(normals_at(G.SCENES[scene](), robj[sel], p), rays.d[sel])
    ok = np.isfinite(n).all(axis=1) & np.isfinite(p).all(axis=1)
    p, n = np.ascontiguousarray(p[ok]), np.ascontiguousarray(n[ok])
    assert len(p) >= N_POINTS - 50, len(p)
    p.setflags(write=False), n.setflags(write=False)
    return p, n, float(np.linalg.norm(p.max(axis=0) - p.min(axis=0)))


@functools.lru_cache(maxsize=None)
def reader(scene, heur):
    return G.Reading(G.SCENES[scene](), G.HEURISTICS[heur])


@functools.lru_cache(maxsize=None)
def ao_reading(scene, heur, bias, samples=S, first=0, n=None, seed=SEED):
    """The reading's closest hits of the AO rays of the scene's points first .. first + n - 1, with index_base = first: (t, obj)."""
    p, nrm, _ = ao_points(scene, heur)
    last = None if n is None else first + n
    o, d = _ao.rays(p[first:last], nrm[first:last], samples, bias, seed, index_base=first)
    return reader(scene, heur).intersect(o, d)


def t_max_cases(extent):
    return {"none": None, "tenth": 0.1 * extent, "nan": float("nan"), "zero": 0.0, "negative": -1.0}


def check(got, want_counts, samples, what):
    vis, cnt = got
    assert cnt.dtype == np.uint32 and vis.dtype == np.float64 and cnt.shape == vis.shape == want_counts.shape
    bad = np.flatnonzero(cnt != want_counts)
    assert len(bad) == 0, (what, len(bad), [(int(i), int(cnt[i]), int(want_counts[i])) for i in bad[:5]])
    assert np.array_equal(bits(vis), bits(_ao.visibility_from(want_counts, samples))), what


# ------------------------------------------------------------------------------------------------------ parity

@pytest.mark.parametrize("bias", [1e-3, 0.0])
@pytest.mark.parametrize("scene,heur", PARITY, ids=IDS)
def test_counts_and_visibility_are_the_readings(scene, heur, bias):
    p, nrm, extent = ao_points(scene, heur)
    t, obj = ao_reading(scene, heur, bias)
    assert (len(p) * S) % 64 != 0
    sc, _ = device_scene(scene, heur)
    for name, t_max in t_max_cases(extent).items():
        want, occ = _ao.counts_from(t, obj, len(p), S, t_max)
        if scene in CONDITION and bias == 1e-3 and name in ("none", "tenth"):
            mixed = int(((want > 0) & (want < S)).sum())
            print(scene, heur, name, "occluded", int(occ.sum()), "unoccluded", int((~occ).sum()), "mixed", mixed)
            assert occ.sum() >= 2000 and (~occ).sum() >= 2000 and mixed >= 400, (int(occ.sum()), int((~occ).sum()), mixed)
        got = sc.ambient_occlusion(p, nrm, samples=S, t_max=t_max, bias=bias, seed=SEED, counts=True)
        check(got, want, S, (scene, heur, bias, name))
        if name in ("nan", "zero", "negative"):
            assert not got[1].any() and (got[0] == 1.0).all()
    # one output alone is the same output
    assert np.array_equal(bits(sc.ambient_occlusion(p, nrm, samples=S, bias=bias, seed=SEED)),
                          bits(_ao.visibility_from(_ao.counts_from(t, obj, len(p), S, None)[0], S)))


@pytest.mark.parametrize("scene", ["mesh1280_light", "soup"])
def test_the_fast_walks_tree_gives_that_trees_counts(scene):
    """The oracle's walk over the tree of single primitives behind their own boxes with nothing culled
    (test_gpu_queries.fast_tree_reading's recipe), on the AO rays."""
    p, nrm, extent = ao_points(scene, "sah1000")
    o, d = _ao.rays(p, nrm, S, 1e-3, SEED)
    objs = G.SCENES[scene]()
    prod = rayrs_amd.Scene(objs, G.T0, G.T1, G.HEURISTICS["sah1000"], HDRI, device=-1)
    osc = _oracle.OracleScene(objs, G.T0, G.T1, G.HEURISTICS["sah1000"], HDRI).use_walk_tree(prod)
    try:
        _oracle.set_cull_margin(float("inf"))
        t, obj = osc.intersect_batch(o, d, G.T0, G.T1, traversal=2, nthreads=16)
    finally:
        _oracle.set_cull_margin(2.0 ** -10)
    sc, _ = device_scene(scene, "sah1000")
    for name, t_max in (("none", None), ("tenth", 0.1 * extent)):
        want, occ = _ao.counts_from(t, obj, len(p), S, t_max)
        assert occ.sum() >= 2000 and (~occ).sum() >= 2000
        check(sc.ambient_occlusion(p, nrm, samples=S, t_max=t_max, bias=1e-3, seed=SEED, fast_traversal=True, counts=True), want, S,
              (scene, "fast", name))


# ------------------------------------------------------------------------------------------------------ the schedule

@pytest.mark.parametrize("n,samples", [(1, 1), (1, 257), (3, 64), (70, 67), (257, 1)])
def test_shapes_where_the_schedule_can_go_wrong(n, samples):
    """A point's samples spanning many refills and several waves, fewer items than a wave, fewer points than a block, S a
    multiple of 64 and not.  The points begin at the first one whose five samples of the parity test are partly occluded,
    and index_base keeps its keys, so a lone point's many samples are not all of one verdict."""
    p, nrm, _ = ao_points("floor_spheres", "sah1000")
    c5 = _ao.counts_from(*ao_reading("floor_spheres", "sah1000", 1e-3), len(p), S, None)[0]
    a = int(np.flatnonzero((c5 > 0) & (c5 < S))[0])
    assert a + n <= len(p)
    t, obj = ao_reading("floor_spheres", "sah1000", 1e-3, samples, a, n)
    want, occ = _ao.counts_from(t, obj, n, samples, None)
    sc, _ = device_scene("floor_spheres", "sah1000")
    check(sc.ambient_occlusion(p[a:a + n], nrm[a:a + n], samples=samples, bias=1e-3, seed=SEED, index_base=a, counts=True), want, samples,
          (n, samples))
    if samples >= S:
        assert occ.any() and not occ.all()


@pytest.mark.parametrize("scene,stack_lds", [("floor_spheres", 0), ("mesh5120", 2)], ids=["floor_spheres", "mesh5120-stacks_in_hbm"])
def test_every_refill_setting_gives_the_same_counts(scene, stack_lds):
    """rayrs_lab_ao_refill: 1 = a wave refills only when none of its lanes walks, 64 = whenever one is idle.  On mesh5120
    with stack_lds = 2 all but two entries of a lane's stack live in the strip the scene keeps for the queries."""
    p, nrm, extent = ao_points(scene, "sah1000")
    t, obj = ao_reading(scene, "sah1000", 1e-3)
    sc, info = device_scene(scene, "sah1000")
    if stack_lds:
        assert info["hot_depth"] > stack_lds and info["wide_depth"] > stack_lds
        sc.lab_set(stack_lds=stack_lds)
    for fast in (False, True):
        first = None
        for refill_below in (1, 32, 64, 0):
            sc.lab_ao_refill(refill_below)
            for t_max in (None, 0.1 * extent):
                got = sc.ambient_occlusion(p, nrm, samples=S, t_max=t_max, bias=1e-3, seed=SEED, fast_traversal=fast, counts=True)
                if not fast:
                    check(got, _ao.counts_from(t, obj, len(p), S, t_max)[0], S, (scene, refill_below, t_max))
                elif first is None or t_max not in first:
                    first = {**(first or {}), t_max: got[1]}
                else:
                    assert np.array_equal(got[1], first[t_max]), (scene, "fast", refill_below, t_max)
    assert sc._L.rayrs_lab_ao_refill(sc._h, 65) == -1


def test_a_slice_with_its_index_base_is_the_slice_of_the_whole_also_across_launches():
    p, nrm, _ = ao_points("soup", "sah1000")
    sc, _ = device_scene("soup", "sah1000")
    kw = dict(samples=S, bias=1e-3, seed=SEED, counts=True)
    vis, cnt = sc.ambient_occlusion(p, nrm, **kw)
    for a, b in ((0, 1), (1, 130), (130, 2049), (2049, len(p))):
        v, c = sc.ambient_occlusion(p[a:b], nrm[a:b], index_base=a, **kw)
        assert np.array_equal(c, cnt[a:b]) and np.array_equal(bits(v), bits(vis[a:b])), (a, b)
    assert not np.array_equal(sc.ambient_occlusion(p[1:130], nrm[1:130], index_base=0, **kw)[1], cnt[1:130])
    # S = 1: a block holds 256 points and a launch 2^20 of them; the points 351 times over is more than that
    reps = 351
    big_p, big_n = np.tile(p, (reps, 1)), np.tile(nrm, (reps, 1))
    n = len(big_p)
    assert n > 1 << 20
    kw1 = dict(samples=1, bias=1e-3, seed=SEED, counts=True)
    vis, cnt = sc.ambient_occlusion(big_p, big_n, **kw1)
    pieces = [sc.ambient_occlusion(big_p[a:b], big_n[a:b], index_base=a, **kw1) for a, b in ((0, 300001), (300001, 1048577), (1048577, n))]
    assert np.array_equal(np.concatenate([c for _, c in pieces]), cnt)
    assert np.array_equal(bits(np.concatenate([v for v, _ in pieces])), bits(vis))
    t, obj = ao_reading("soup", "sah1000", 1e-3, 1)
    want, occ = _ao.counts_from(t, obj, len(p), 1, None)
    assert occ.sum() >= 500 and (~occ).sum() >= 500
    assert np.array_equal(cnt[:len(p)], want)
    assert 0 < cnt[len(p):].sum() < n - len(p)   # (other indices, other rays: not a copy of the first 3,000)
    # none: RAYRS_OK, nothing launched, empty answers
    v0, c0 = sc.ambient_occlusion(np.zeros((0, 3)), np.zeros((0, 3)), **kw)
    assert v0.shape == (0,) and c0.shape == (0,)


def test_device_tensors_on_a_stream_give_the_host_paths_bits():
    """tests/_ao_torch_child.py, in a process of its own (torch has to be imported before the library is loaded)."""
    pytest.importorskip("torch")
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_ao_torch_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "device path ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


# ------------------------------------------------------------------------------------------------------ the image form

def mesh3(cam=((0.0, 1.2, 8.0), (0.0, 1.0, 0.0), (0.0, 1.5, 0.0), 50.0, 1.0, 1.0, 100)):
    """scenes.mesh_scene(3, area_light=True) seen from near the floor, so that the upper rows look past it."""
    _, objs, heur = scenes.mesh_scene(3, area_light=True)
    return cam, objs, heur


def floor_spheres_view():
    return ((0.0, 1.2, 7.0), (0.0, 1.0, 0.0), (0.0, 1.2, 0.0), 50.0, 1.0, 1.0, 100), G.SCENES["floor_spheres"](), G.HEURISTICS["sah1000"]


@pytest.mark.parametrize("view", [floor_spheres_view, mesh3], ids=["floor_spheres", "mesh3_light"])
def test_the_plane_is_the_oracles_first_hit_and_the_reading_there(view):
    """44 x 28: edge tiles on both axes.  Expected from the oracle alone: OracleCamera.primary_ray with the sample-0 key,
    OracleScene.intersect, the normal from the object table, the turn rule, then tests/_ao.py."""
    cam_args, objs, heur = view()
    W, H, samples, seed, ao_seed, bias = 44, 28, 4, 77, 0xA0, 1e-4
    args = scenes.camera_for_resolution(cam_args, W, H)
    cam, ocam = rayrs_amd.Camera(*args), _oracle.OracleCamera(*args)
    assert (cam.x_pixels(), cam.y_pixels()) == (W, H) == (ocam.x_pixels(), ocam.y_pixels())
    osc = _oracle.OracleScene(objs, G.T0, G.T1, heur, HDRI)
    idx, o_hit, d_hit, t_hit, obj_hit = [], [], [], [], []
    for r in range(H):
        for c in range(W):
            o, d, _ = ocam.primary_ray(H - r, W - c, _ao.path_key(seed, r * W + c, 0))
            k, t = osc.intersect(o, d, G.T0, G.T1)
            if k >= 0:
                idx.append(r * W + c), o_hit.append(o), d_hit.append(d), t_hit.append(t), obj_hit.append(k)
    idx, o_hit, d_hit, t_hit, obj_hit = (np.array(a) for a in (idx, o_hit, d_hit, t_hit, obj_hit))
    assert len(idx) >= 100 and W * H - len(idx) >= 100, len(idx)
    p = np.stack(G.point(G.vec(o_hit), G.vec(d_hit), t_hit), axis=1)
    n = _ao.turned(normals_at(objs, obj_hit, p), d_hit)
    ao_o, ao_d = _ao.rays(p, n, samples, bias, ao_seed, indices=idx)
    t, obj = G.Reading(objs, heur).intersect(ao_o, ao_d)
    sc = rayrs_amd.Scene(objs, G.T0, G.T1, heur, HDRI, device=0)
    for t_max in (None, 1.0):
        want = np.zeros(W * H, dtype=np.uint32)
        want[idx], occ = _ao.counts_from(t, obj, len(idx), samples, t_max)
        assert occ.any() and not occ.all()
        vis, cnt = rayrs_amd.render_ao(sc, cam, samples=samples, t_max=t_max, bias=bias, seed=seed, ao_seed=ao_seed, counts=True)
        assert vis.shape == (H, W) and cnt.shape == (H, W)
        check((vis.reshape(-1), cnt.reshape(-1)), want, samples, (view.__name__, t_max))
        miss = np.ones(W * H, dtype=bool)
        miss[idx] = False
        assert (vis.reshape(-1)[miss] == 1.0).all() and not cnt.reshape(-1)[miss].any()
    assert np.array_equal(bits(rayrs_amd.render_ao(sc, cam, samples=samples, t_max=1.0, bias=bias, seed=seed, ao_seed=ao_seed)), bits(vis))


def test_a_render_is_the_same_before_and_after_a_batch_of_ao_calls():
    cam_args, objs, heur = scenes.mesh_scene(3, area_light=True)
    sc = rayrs_amd.Scene(objs, G.T0, G.T1, heur, HDRI, device=0)
    cam = rayrs_amd.Camera(*scenes.camera_for_resolution(cam_args, 48, 32))
    before, st0 = rayrs_amd.render(sc, cam, 4, out_f64=True)
    p, nrm, extent = ao_points("mesh1280_light", "sah1000")
    for fast in (False, True):
        sc.ambient_occlusion(p, nrm, samples=S, bias=1e-3, fast_traversal=fast)
        sc.ambient_occlusion(p, nrm, samples=S, bias=1e-3, t_max=0.1 * extent, fast_traversal=fast)
        rayrs_amd.render_ao(sc, cam, samples=4, bias=1e-4, fast_traversal=fast)
    after, st1 = rayrs_amd.render(sc, cam, 4, out_f64=True)
    assert before.tobytes() == after.tobytes()
    assert st0["rays"] == st1["rays"] and st0["paths"] == st1["paths"]


# ------------------------------------------------------------------------------------------------------ the command line

def run_cli(tmp, sub, args):
    d = tmp / sub
    d.mkdir()
    r = subprocess.run([CLI, str(tmp / "env.hdr"), "4", "--seed", "77", "--scene", "diffuse_single_sphere"] + args, cwd=d,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return d


def test_the_command_line_writes_the_ao_plane_and_the_same_ordinary_files(tmp_path):
    io.save_hdr(tmp_path / "env.hdr", procedural.make_hdri(128, 64))
    name = "diffuse_single_sphere"
    plain = run_cli(tmp_path, "without", [])
    with_ao = run_cli(tmp_path, "with", ["--ao", "8"])
    radius = run_cli(tmp_path, "radius", ["--ao-radius", "1.5", "--ao"])
    for f in (name + ".png", name + ".hdr"):
        assert (plain / f).read_bytes() == (with_ao / f).read_bytes() == (radius / f).read_bytes(), f
    assert sorted(os.listdir(plain)) == [name + ".hdr", name + ".png"]
    assert sorted(os.listdir(with_ao)) == sorted([name + ".hdr", name + ".png", name + "_ao.hdr", name + "_ao.png"])
    assert (with_ao / (name + "_ao.png")).stat().st_size > 64
    cam_args, objs, heur = scenes.diffuse_single_sphere()
    scene, cam = rayrs_amd.Scene(objs, 1e-6, 1e6, heur, io.load_hdr(tmp_path / "env.hdr"), device=0), rayrs_amd.Camera(*cam_args)
    b = scene.info()["root_box"]
    dx, dy, dz = b[1] - b[0], b[3] - b[2], b[5] - b[4]
    bias = 1e-6 * float(np.sqrt(dx * dx + dy * dy + dz * dz))
    for d, samples, t_max in ((with_ao, 8, None), (radius, 16, 1.5)):
        vis = rayrs_amd.render_ao(scene, cam, samples=samples, t_max=t_max, bias=bias, seed=77, ao_seed=0xA0)
        assert vis.min() < 1.0 and vis.max() == 1.0
        io.save_hdr(tmp_path / "want.hdr", np.repeat(vis[..., None], 3, axis=2).astype(np.float32))
        assert np.array_equal(io.load_hdr(d / (name + "_ao.hdr")), io.load_hdr(tmp_path / "want.hdr")), samples
    r = subprocess.run([CLI, str(tmp_path / "env.hdr"), "4", "--ao", "0"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 2 and "--ao" in r.stderr and not (tmp_path / "material_test.png").exists()
