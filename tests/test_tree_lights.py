"""A mesh-light group chosen by a light tree (include/rayrs_hip.h LIGHT TREE) without a GPU: the entry points are declared,
exported and bound; the nodes, powers, paths, tree_sample, tree_probability and p_tri of the library's host calls are the
plain-Python reading's (tests/_tree.py) bit for bit, at points on a listed triangle and with NaN and infinite components too;
tree_probability is the p tree_sample arrived with; the probabilities of one point sum to one; p_sel is the probability of the
draws; every refusal that is decided before the device is touched comes in the header's order, the film's and the bake's among
them; the kernels keep their resources; and the reading of the turn is held to what makes it worth comparing with: its
irradiance has the unlit mean, and where one of two equal panels is thirty times farther its variance is below the area group's."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _direct
import _geometry_reading as G
import _mesh
import _tree
import rayrs_amd
from rayrs_amd import _ffi, procedural
from rayrs_amd.api import Axis, BvhHeuristic, Emission, Material, Object
from test_direct import HIPCC, compile_asm, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_CALLS = ["rayrs_mesh_lights_create_tree", "rayrs_mesh_lights_tree_nodes", "rayrs_mesh_lights_tree_entries",
              "rayrs_mesh_lights_tree_sample", "rayrs_mesh_lights_tree_probability"]
INVALID_ARG, NO_DEVICE, UNSUPPORTED = -1, -4, -5
Z_NEAR, Z_FAR = 1e-6, 1e6
F = np.float64
STUDIO = procedural.make_studio_hdri(9, 5)
WHITE = Material.LambertianDiffuse((0.8, 0.8, 0.8))
PALETTE = [Emission.new(4.0, (1.0, 0.9, 0.8)), Emission.new(64.0, (0.2, 1.0, 0.5)), Emission.Dark(), Emission.new(0.5, (1.0, 1.0, 1.0))]
LAST = F(1.0) - F(2.0) ** -53   # the largest f64 below 1
NONE = 0xFFFFFFFF


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def test_the_header_states_the_operation_and_the_binding_declares_it():
    head = open(os.path.join(ROOT, "include", "rayrs_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", head, flags=re.S)
    L = _ffi.lib()
    for name in HOST_CALLS:
        assert re.search(rf"\bint {name}\s*\(", code), name
        assert name in _ffi.SYMBOLS and hasattr(L, name) and getattr(L, name).argtypes, name
    assert L.rayrs_mesh_lights_create_tree.argtypes == L.rayrs_mesh_lights_create.argtypes
    text = re.sub(r"\s+", " ", re.sub(r"\s*\n \*\s*", " ", head))
    assert text.index("MESH-LIT FILMS AND BAKES.") < text.index("LIGHT TREE, specified to the operation") < text.index("The boundary's version")
    for line in ("w_j = A_j * ((e_r + e_g) + e_b)", "m = (lo + hi) * 0.5; r2 = (hi - m).mag2(); W = W_left + W_right",
                 "I_c = W_c > 0.0 ? W_c / rr_max(|x - m_c|^2, r2_c) : 0.0", "P_l = I_l / s if s > 0.0 && s < +inf, else W_l / (W_l + W_r)",
                 "P_r = 1.0 - P_l", "r = rr_min(u, 1.0)", "a NaN comparison goes RIGHT",
                 "p_tri = ((position - q).mag2() / (|n_j . l_s| * A_j)) * p_sel",
                 "p = ((o - ray.point(t)).mag2() / (|normal . d| * A_j)) * tree_probability(o, j)", "Why it is unbiased",
                 "REFUSE a tree handle"):
        assert line in text, line


# ---- the host calls against the reading

def tri_list(n, seed):
    """(objects, the listed triangles): a floor, then n triangles of assorted sizes, tilts and emissions -- every fourth dark --;
    from n = 2 on entries 0 and 1 are the same triangle with two emissions, so their centroid keys are equal, and from n = 3 on
    one entry in the middle has area zero and emits.  The list is not in scene order."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-3.0, 3.0, size=(n, 1, 3)) + (0.0, 4.0, 0.0)
    verts = centre + rng.normal(size=(n, 3, 3)) * rng.uniform(0.05, 0.6, size=(n, 1, 1))
    if n >= 2:
        verts[1] = verts[0]
    if n >= 3:
        verts[max(n // 2, 2)][2] = verts[max(n // 2, 2)][1]
    em = [PALETTE[(k + (k >= 2)) % 4] for k in range(n)]   # (entries 0 and 1 emit, unequally; so does the one without area)
    objs = [Object.plane(Axis.Y, -5.0, 5.0, -5.0, 5.0, 0.0, WHITE, Emission.Dark())]
    objs += [Object.triangle(tuple(v[0]), tuple(v[1]), tuple(v[2]), WHITE, e) for v, e in zip(verts, em)]
    order = list(range(1, n + 1))
    return objs, order[:2] + order[2:][::-1]


def emit_sum(T, scene, j):
    return sum(_tree.emit_of(T.prims_list[T.tris[j]]))


def positions_for(T, rng, n):
    """Ordinary points below the triangles; points ON listed triangles (a vertex, a centroid: the r2 clamp); a third with a NaN
    or an infinite component."""
    pos = rng.uniform(-4.0, 4.0, size=(n, 3)) * (1.0, 0.0, 1.0) + (0.0, 0.5, 0.0)
    for k in range(0, n, 5):
        p1, p2, p3 = T.p[k % len(T)]
        pos[k] = p1 if k % 2 else (np.array(p1) + np.array(p2) + np.array(p3)) / 3.0
    bad = (np.nan, np.inf, -np.inf)
    for k in range(1, n, 3):
        pos[k, k % 3] = bad[(k // 3) % 3]
    return pos


@pytest.fixture(scope="module")
def tables():
    out = {}
    for n in (1, 2, 3, 65, 1025):
        objs, tris = tri_list(n, 100 + n)
        scene = rayrs_amd.Scene(objs, Z_NEAR, Z_FAR, BvhHeuristic.Sah(1000), STUDIO, device=-1)
        out[n] = (scene, scene.mesh_lights(tris, tree=True), _tree.Tree(G.Prims(objs), tris))
    yield out
    for scene, group, _ in out.values():
        group.close()
        scene.close()


@pytest.mark.parametrize("n", [1, 2, 3, 65, 1025])
def test_nodes_powers_paths_sample_and_probability_are_the_readings(tables, n):
    scene, group, T = tables[n]
    assert group.tree and len(group) == len(T) == n
    assert np.array_equal(bits(group.areas()), bits(np.array(T.A)))
    assert np.array_equal(bits(group.powers()), bits(np.array(T.w)))
    path, depth = group.paths()
    assert np.array_equal(path, np.array(T.path, dtype=np.uint32)) and np.array_equal(depth, np.array(T.depth, dtype=np.uint32))
    assert depth.max() == int(np.ceil(np.log2(n))) if n > 1 else depth.max() == 0
    mrw, right, entry = group.nodes()
    assert len(T.nodes) == 2 * n - 1 == len(mrw)
    assert np.array_equal(bits(mrw), bits(np.array([list(m) + [r2, W] for m, r2, W, _, _ in T.nodes])))
    assert np.array_equal(right, np.array([NONE if r is None else r for _, _, _, r, _ in T.nodes], dtype=np.uint32))
    assert np.array_equal(entry, np.array([NONE if e is None else e for _, _, _, _, e in T.nodes], dtype=np.uint32))
    assert sorted(e for e in entry if e != NONE) == list(range(n))
    if n >= 2:   # equal keys: the tie goes by list index, entry 0 left of entry 1 wherever they part
        assert T.key[0] == T.key[1] and T.w[0] != T.w[1]
        k = next(k for k in range(32) if (T.path[0] >> k) & 1 != (T.path[1] >> k) & 1)
        assert (T.path[0] >> k) & 1 == 0 and (T.path[1] >> k) & 1 == 1
    if n >= 3:
        flat = [k for k in range(n) if T.A[k] == 0.0]
        assert len(flat) == 1 and T.w[flat[0]] == 0.0 and emit_sum(T, scene, flat[0]) > 0.0
        assert n == 3 or any(w == 0.0 and a > 0.0 for w, a in zip(T.w, T.A))   # (and a dark entry with area)
    rng = np.random.default_rng(n)
    m = 120 if n > 100 else 240
    u = rng.random((m, 2))
    u[:6] = [(0.0, 0.0), (LAST, LAST), (0.0, LAST), (LAST, 0.0), (0.5, 0.0), (0.5, LAST)]
    pos = positions_for(T, rng, m)
    j, q, p_sel = group.sample(u, pos)
    want = [T.tree_sample(_mesh.f3(pos[k]), F(u[k, 0]), F(u[k, 1])) for k in range(m)]
    assert (j < n).all()   # the descent ends inside the table, whatever the point
    assert np.array_equal(j, np.array([w[0] for w in want], dtype=np.uint32))
    assert np.array_equal(bits(q), bits(np.array([w[1] for w in want])))
    assert np.array_equal(bits(p_sel), bits(np.array([w[2] for w in want])))
    finite = np.isfinite(pos).all(axis=1)
    assert (np.array(T.w)[j[finite]] > 0.0).all()            # an entry without power is never drawn
    assert (p_sel[finite] > 0.0).all() and (p_sel[finite] <= 1.0).all()
    jj = rng.integers(0, n, size=m).astype(np.uint32)
    p = group.probability(pos, jj)
    assert np.array_equal(bits(p), bits(np.array([T.tree_probability(_mesh.f3(pos[k]), int(jj[k])) for k in range(m)])))
    d = group.density(pos, j, q)
    assert np.array_equal(bits(d), bits(np.array([T.tree_aim(_mesh.f3(pos[k]), int(j[k]), want[k][1], want[k][2])[1] for k in range(m)])))
    if n > 1:   # the r2 clamp was exercised: some point is nearer to a node's middle than its half diagonal
        assert any(G.dot(G.sub(_mesh.f3(pos[k]), nd[0]), G.sub(_mesh.f3(pos[k]), nd[0])) < nd[1] for k in range(0, m, 5) for nd in T.nodes)
    with pytest.raises(_ffi.RayrsError) as e:   # mesh_sample has no position
        group.sample(u)
    assert e.value.status == UNSUPPORTED


@pytest.mark.parametrize("n", [2, 65, 1025])
def test_probability_is_the_p_sample_arrived_with(tables, n):
    scene, group, T = tables[n]
    rng = np.random.default_rng(7 * n)
    m = 4000
    pos = positions_for(T, rng, m)
    j, q, p_sel = group.sample(rng.random((m, 2)), pos)
    assert np.array_equal(bits(group.probability(pos, j)), bits(p_sel))
    assert len(np.unique(j)) >= min(n, 40) // 2


def test_the_probabilities_of_a_point_sum_to_one(tables):
    """Each term carries about depth * 3 ulp and the sum about N ulp, so it is 1 to about 1e-13 at N = 1025: the bound is 1e-12.
    An entry without power has probability 0.0, or NaN where its whole sibling subtree is without power (0 / 0, the header)."""
    scene, group, T = tables[1025]
    w = np.array(T.w)
    for x in ((0.3, 0.5, 0.2), (-3.5, 0.0, 3.0), (0.0, 4.0, 0.0), tuple(T.p[7][0]), (50.0, 80.0, -20.0)):
        p = group.probability(np.tile(x, (1025, 1)), np.arange(1025, dtype=np.uint32))
        assert (np.isfinite(p[w > 0.0]) & (p[w > 0.0] > 0.0)).all()
        assert (np.isnan(p[w == 0.0]) | (p[w == 0.0] == 0.0)).all()
        total = np.nansum(p)
        print("x", x, "sum - 1", total - 1.0)
        assert abs(total - 1.0) <= 1e-12


def test_p_sel_is_the_probability_of_the_draws(tables):
    """For a fixed x, E[A_j / p_sel] over the draws is the summed area of the entries that can be drawn.  The draws are the
    library's, which are the reading's bit for bit (above); x is a floor point a few units from every triangle, where no single
    entry's ratio dominates the variance."""
    scene, group, T = tables[65]
    n = 1 << 16
    x = (0.3, 0.5, 0.2)
    j, q, p_sel = group.sample(np.random.default_rng(5).random((n, 2)), np.tile(x, (n, 1)))
    ratio = np.array(T.A)[j] / p_sel
    want = sum(a for a, w in zip(T.A, T.w) if w > 0.0)
    mean, se = ratio.mean(), ratio.std(ddof=1) / np.sqrt(n)
    print("area of what can be drawn", want, "mean A_j / p_sel", mean, "+-", se)
    assert np.isfinite(ratio).all() and abs(mean - want) <= 5.0 * se and se < 0.02 * want


# ---- refusals

def test_creations_refusals_come_in_the_headers_order():
    """rayrs_mesh_lights_create's, in its order (tests/test_mesh_lights.py's scene and cases), then the three the tree adds."""
    from test_mesh_lights import refusal_scene
    L = _ffi.lib()

    def create(scene, tris, n=None, no_scene=False, no_out=False):
        h = C.c_void_p()
        arr = None if tris is None else np.array(tris, dtype=np.uint32)
        st = L.rayrs_mesh_lights_create_tree(None if no_scene else scene._h, None if arr is None or len(arr) == 0 and n is None else arr.ctypes.data,
                                             (0 if arr is None else len(arr)) if n is None else n, None if no_out else C.byref(h))
        if st == 0:
            L.rayrs_mesh_lights_destroy(h)
        return st
    scene = refusal_scene()
    for bad in (dict(no_scene=True), dict(no_out=True)):
        assert create(scene, [6], **bad) == INVALID_ARG and create(scene, [3], **bad) == INVALID_ARG, bad
    assert create(scene, None, n=2) == INVALID_ARG
    for tris in ([6, 12], [12], [3, 100], [6, 6], [6, 7, 6], [3, 3], [8, 8], [0xffffffff]):
        assert create(scene, tris) == INVALID_ARG, tris
    assert create(scene, list(range(13)), n=1 << 31) == INVALID_ARG
    for tris in ([3], [6, 0], [4, 8], [8], [6, 8], [9], [7, 9], [10], [6, 10, 8]):
        assert create(scene, tris) == UNSUPPORTED, tris
    for tris in ([7], [7, 10]):               # area, but no power: a group the plain creator takes
        assert create(scene, tris) == UNSUPPORTED, tris
    for tris in ([], [6], [6, 7], [6, 10], [11, 7, 6], [10, 6]):
        assert create(scene, tris) == 0, tris
    assert create(scene, None) == 0
    scene.close()
    # an emission that is not finite (an infinite strength, and inf * 0 in a channel), and a total power that is not
    t = lambda dx, em: Object.triangle((dx, 3.0, 0.0), (dx + 0.5, 3.0, 0.0), (dx, 3.0, 0.5), WHITE, em)
    objs = [t(0.0, PALETTE[0]), t(1.0, Emission.new(np.inf, (1.0, 1.0, 1.0))), t(2.0, Emission.new(np.inf, (1.0, 0.0, 1.0))),
            t(3.0, Emission.new(1e308, (1.0, 1.0, 1.0)))]
    scene = rayrs_amd.Scene(objs, Z_NEAR, Z_FAR, BvhHeuristic.Sah(1000), STUDIO, device=-1)
    for tris in ([1], [2], [0, 1], [3], [0, 3]):
        assert create(scene, tris) == UNSUPPORTED, tris
        scene.mesh_lights(tris).close()       # (the plain creator takes them)
    assert create(scene, [0]) == 0
    scene.close()


def test_the_host_calls_refusals_and_the_films_and_the_bakes():
    L = _ffi.lib()
    objs, tris = tri_list(3, 1)
    scene = rayrs_amd.Scene(objs, Z_NEAR, Z_FAR, BvhHeuristic.Sah(1000), STUDIO, device=-1)
    other = rayrs_amd.Scene(objs, Z_NEAR, Z_FAR, BvhHeuristic.Sah(1000), STUDIO, device=-1)
    tree, empty, area, foreign = (scene.mesh_lights(tris, tree=True), scene.mesh_lights([], tree=True), scene.mesh_lights(tris),
                                  other.mesh_lights(tris, tree=True))
    P = lambda x: x.ctypes.data
    x, u, j, q, p = np.zeros((1, 3)), np.zeros((1, 2)), np.zeros(1, dtype=np.uint32), np.zeros((1, 3)), np.zeros(1)
    big, five, words = np.array([3], dtype=np.uint32), np.zeros((5, 5)), np.zeros(5, dtype=np.uint32)
    assert L.rayrs_mesh_lights_tree_nodes(None, P(five), P(words), P(words)) == INVALID_ARG
    assert L.rayrs_mesh_lights_tree_nodes(tree._h, None, None, None) == INVALID_ARG
    assert L.rayrs_mesh_lights_tree_nodes(area._h, P(five), None, None) == UNSUPPORTED
    assert L.rayrs_mesh_lights_tree_nodes(tree._h, P(five), None, None) == 0 and L.rayrs_mesh_lights_tree_nodes(empty._h, P(five), None, None) == 0
    assert L.rayrs_mesh_lights_tree_entries(tree._h, None, None, None) == INVALID_ARG
    assert L.rayrs_mesh_lights_tree_entries(area._h, P(p), None, None) == UNSUPPORTED
    assert L.rayrs_mesh_lights_tree_sample(tree._h, None, P(u), 1, P(j), P(q), P(p)) == INVALID_ARG
    assert L.rayrs_mesh_lights_tree_sample(area._h, P(x), P(u), 1, P(j), P(q), P(p)) == UNSUPPORTED
    assert L.rayrs_mesh_lights_tree_sample(empty._h, P(x), P(u), 1, P(j), P(q), P(p)) == UNSUPPORTED
    assert L.rayrs_mesh_lights_tree_sample(tree._h, P(x), P(u), 1, P(j), P(q), P(p)) == 0
    assert L.rayrs_mesh_lights_tree_probability(tree._h, P(x), P(big), 1, P(p)) == INVALID_ARG   # (j is not below N)
    assert L.rayrs_mesh_lights_tree_probability(area._h, P(x), P(j), 1, P(p)) == UNSUPPORTED
    assert L.rayrs_mesh_lights_tree_probability(empty._h, P(x), P(j), 0, P(p)) == UNSUPPORTED
    assert L.rayrs_mesh_lights_tree_probability(tree._h, P(x), P(j), 1, P(p)) == 0
    assert L.rayrs_mesh_lights_sample(tree._h, P(u), 1, P(j), P(q)) == UNSUPPORTED
    assert L.rayrs_mesh_lights_density(tree._h, P(x), P(big), P(q), 1, P(p)) == INVALID_ARG
    assert L.rayrs_mesh_lights_density(tree._h, P(x), P(j), P(q), 1, P(p)) == 0
    tot = C.c_double(-1.0)
    assert L.rayrs_mesh_lights_table(tree._h, None, C.addressof(tot)) == 0 and tot.value == area.total
    with pytest.raises(ValueError):
        area.powers()
    with pytest.raises(ValueError):
        area.sample(u, x)
    # the queries take a tree handle to the device's door; the film and the bake refuse it before that, in the RAYRS_UNSUPPORTED
    # group: behind a handle of another scene, ahead of RAYRS_NO_DEVICE
    pts, up = np.zeros((4, 3)), np.tile((0.0, 1.0, 0.0), (4, 1))
    cam = rayrs_amd.Camera((0.0, 2.2, 7.0), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), 50.0, 24 / 25.4 + 1e-9, 16 / 25.4 + 1e-9, 10)
    for group, status in ((area, NO_DEVICE), (tree, UNSUPPORTED), (empty, UNSUPPORTED), (foreign, INVALID_ARG)):
        for make in (lambda: scene.irradiance(pts, up, samples=2, lights=[], direct=True, mesh=group),
                     lambda: scene.radiance(pts, up, samples=2, lights=[], direct=True, mesh=group),
                     lambda: rayrs_amd.render_lit(scene, cam, 1, [], direct=True, mesh=group)):
            with pytest.raises(_ffi.RayrsError) as e:
                make()
            assert e.value.status == (INVALID_ARG if group is foreign else NO_DEVICE)
        for sky in (False, True):
            with pytest.raises(_ffi.RayrsError) as e:
                rayrs_amd.Film(scene, cam, lights=[rayrs_amd.SKY] if sky else [], direct=True, mesh=group)
            assert e.value.status == status, (status, str(e.value))
            with pytest.raises(_ffi.RayrsError) as e:
                rayrs_amd.Bake(scene, pts, up, lights=[rayrs_amd.SKY] if sky else [], direct=True, mesh=group)
            assert e.value.status == status, (status, str(e.value))
    for h in (tree, empty, area, foreign):
        h.close()
    scene.close()
    other.close()


# ---- kernel resources: the rule of the mesh kernels (tests/test_mesh_lights.py)
VGPR_BOUND = 256


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_the_tree_kernels_use_no_scratch_and_keep_two_waves_per_simd(tmp_path):
    res = kernel_resources(compile_asm("radiance_tree.hip", tmp_path))
    path = {n: r for n, r in res.items() if "radiance_tree_kernel" in n}
    resolve = {n: r for n, r in res.items() if "radiance_tree_resolve_kernel" in n}
    assert len(path) == 24 and len(resolve) == 1 and len(res) == 25   # COMPACT x EXACT x SKY x the three starts; the resolve
    for name, (vgpr, scratch, lds) in res.items():
        print(name, vgpr, scratch, lds)
        assert vgpr <= VGPR_BOUND and scratch == 0 and lds == 0, (name, vgpr, scratch, lds)   # (the stacks are dynamic LDS)


# ---- the reading is unbiased, and pays

def test_tree_irradiance_has_the_unlit_mean():
    """tests/test_mesh_lights.py's comparison for the tree's reading: tests/_mesh.py's room under the studio map, the means with
    the lamps and the group, with the sky as well, and with the group alone each agree with the unlit mean within 4 combined
    standard errors in every channel."""
    cam, objs, heur, names = _mesh.mesh_room()
    R = _tree.Reading(objs, Z_NEAR, Z_FAR, heur, STUDIO, names["group"])
    D = _direct.Reading(objs, Z_NEAR, Z_FAR, heur, STUDIO, osc=R.osc)
    points = np.array([(0.0, 0.0, 0.0), (-3.0, 0.0, 3.0)])
    normals = np.tile((0.0, 1.0, 0.0), (len(points), 1))
    lamps = [names["sphere_lamp"], names["rect_lamp"]]
    s_lit, s_unlit = 1500, 6000
    runs = (("lamps + group", _tree.irradiance_paths(R, points, normals, s_lit, 1e-4, 50, 11, lamps)),
            ("lamps + group + sky", _tree.irradiance_paths(R, points, normals, s_lit, 1e-4, 50, 11, lamps + [rayrs_amd.SKY])),
            ("group alone", _tree.irradiance_paths(R, points, normals, s_lit, 1e-4, 50, 13, [])))
    unlit, uq = _direct.irradiance_paths(D, points, normals, s_unlit, 1e-4, 50, 12, [])
    assert np.isfinite(unlit).all() and all(np.isfinite(x).all() for _, (x, _) in runs)
    for i in range(len(points)):
        mu, vu = unlit[i].mean(axis=0), unlit[i].var(axis=0, ddof=1)
        for what, (x, q) in runs:
            m, v = x[i].mean(axis=0), x[i].var(axis=0, ddof=1)
            se = np.sqrt(v / s_lit + vu / s_unlit)
            print("point", points[i].tolist(), what, m, "unlit", mu, "difference / se", (m - mu) / se, "variance / unlit", v / vu)
            assert (np.abs(m - mu) <= 4.0 * se).all(), (i, what, m, mu, se)


def two_panels():
    """A floor, and two equal emissive panels facing down: one a unit above the origin, one thirty units along x at the same
    height.  Uniform choice spends half its draws on a panel that contributes about 1 / 900 of the light at the origin."""
    floor = Object.plane(Axis.Y, -40.0, 40.0, -40.0, 40.0, 0.0, WHITE, Emission.Dark())
    objs, tris = [floor], []
    for dx in (0.0, 30.0):
        v = np.array([(dx - 0.25, 1.0, -0.25), (dx + 0.25, 1.0, -0.25), (dx + 0.25, 1.0, 0.25), (dx - 0.25, 1.0, 0.25)])
        objs += Object.from_triangles(v, np.array([(0, 1, 2), (0, 2, 3)], dtype=np.uint32), WHITE, Emission.new(20.0, (1.0, 1.0, 1.0)))
    return objs, [1, 2, 3, 4]


def test_the_tree_pays_where_one_panel_is_far():
    objs, tris = two_panels()
    black = np.zeros((5, 9, 3), dtype=np.float32)
    heur = BvhHeuristic.Sah(1000)
    T = _tree.Reading(objs, Z_NEAR, Z_FAR, heur, black, tris)
    A = _mesh.Reading(objs, Z_NEAR, Z_FAR, heur, black, tris, osc=T.osc)
    point, normal, s = np.array([(0.1, 0.0, 0.05)]), np.array([(0.0, 1.0, 0.0)]), 1500
    tree, _ = _tree.irradiance_paths(T, point, normal, s, 1e-4, 4, 21, [])
    area, _ = _mesh.irradiance_paths(A, point, normal, s, 1e-4, 4, 21, [])
    mt, ma = tree[0].mean(axis=0), area[0].mean(axis=0)
    vt, va = tree[0].var(axis=0, ddof=1), area[0].var(axis=0, ddof=1)
    print("means", mt, ma, "variance tree / area", vt / va)
    assert (np.abs(mt - ma) <= 4.0 * np.sqrt((vt + va) / s)).all()
    assert (vt < va).all()
