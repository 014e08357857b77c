"""SH probes (include/rayrs_hip.h SH PROBES) on the GPU, bit for bit and count for count against the plain-Python reading of the
operation (tests/_probes.py): the unlit paths on tests/test_gpu_radiance.py's families -- an open scene, a closed room, a scene of
compact records -- on both walks, every lighting on the rooms the four direct-lighting test files build, the shapes where the
item order or the projection can go wrong (one sample, one probe, more items than a wave, a launch and one probe, a probe whose
chunks lie in two rounds of the projection), slices, device tensors, and the neighbours on the shared scratch."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import _probes
import rayrs_amd
import test_gpu_direct
import test_gpu_mesh_lights
import test_gpu_sky
import test_gpu_tree_lights
from rayrs_amd import SKY
from test_gpu_radiance import SEED, Z_FAR, bits, family

pytestmark = pytest.mark.gpu

S = 5
# probes of the families: above and between material_test's spheres (open: the map is overhead); inside the closed white room,
# the last at the centre of its glass sphere; around mesh3_light's blob, under its lamp
POINTS = {
    "material_test": np.array([(-3.0, 1.5, 1.0), (0.4, 1.6, 2.0), (4.0, 2.5, -1.0)]),
    "white_room": np.array([(0.0, 0.0, 0.0), (-1.2, 1.3, 2.1), (0.8, -0.9, -0.6)]),
    "mesh3_light": np.array([(1.5, 1.0, 1.5), (0.0, 3.0, 0.2), (-2.0, 0.5, 1.0)]),
}
BOUNCES = {"material_test": 50, "white_room": 12, "mesh3_light": 50}   # (the white room's paths all run to the budget)
ROOM_POINTS = np.array([(0.3, 0.25, 0.4), (-0.6, 0.5, -1.2)])   # tests/_lit.py's lit room and tests/_mesh.py's: low over the floor


@functools.lru_cache(maxsize=None)
def expected(name, fast=False, samples=S, n=3, first=0, max_bounces=None):
    """The reading's unlit paths of the family's probes first .. first + n - 1 with index_base = first."""
    f = family(name)
    return _probes.unlit_paths(f.fast if fast else f.osc, POINTS[name][first:first + n], samples,
                               BOUNCES[name] if max_bounces is None else max_bounces, SEED, first, traversal=2 if fast else 0)


def check(got, paths, chunk, what, finite=True):
    coeffs, cnt = got
    values, queries, w = paths
    want, want_cnt = _probes.answers(values, queries, w, chunk)
    assert coeffs.dtype == np.float64 and cnt.dtype == np.uint32 and coeffs.shape == want.shape and cnt.shape == want_cnt.shape, what
    bad = np.flatnonzero(cnt != want_cnt)
    assert len(bad) == 0, (what, "queries", [(int(i), int(cnt[i]), int(want_cnt[i])) for i in bad[:5]])
    if finite:
        assert np.isfinite(want).all(), what
        bad = np.flatnonzero((bits(coeffs) != bits(want)).any(axis=(1, 2)))
        assert len(bad) == 0, (what, "coeffs", len(bad), [(int(i), coeffs[i].tolist(), want[i].tolist()) for i in bad[:2]])
    else:
        assert _probes.same_or_nan(coeffs, want), what
    return want, want_cnt


# ------------------------------------------------------------------------------------------------------ parity

@pytest.mark.parametrize("fast", [False, True], ids=["default", "fast"])
@pytest.mark.parametrize("name", ["material_test", "white_room", "mesh3_light"])
def test_coefficients_and_queries_are_the_readings(name, fast):
    f = family(name)
    kw = dict(max_bounces=BOUNCES[name], seed=SEED, fast_traversal=fast, queries=True)
    paths = expected(name, fast)
    lone = expected(name, fast, samples=65, n=1, first=1)
    one = expected(name, fast, samples=1)
    # the conditions that keep the comparison from being vacuous, from the reading alone
    first_q = np.concatenate([paths[1].ravel(), lone[1].ravel()])
    assert max(paths[1].max(), lone[1].max(), one[1].max()) >= 4, name
    differ = int((bits(_probes.answers(*paths, 0)[0]) != bits(_probes.answers(*paths, 2)[0])).any(axis=(1, 2)).sum())
    assert differ >= 1, name
    if name == "material_test":   # open: a first ray that escapes makes one query and carries the map's radiance
        rays = [(POINTS[name][i], paths[2][i, s]) for i in range(3) for s in range(S)] + [(POINTS[name][1], lone[2][0, s]) for s in range(65)]
        hit = np.array([f.osc.intersect(o, d, f.z_near, Z_FAR)[0] >= 0 for o, d in rays])
        print(name, "first rays", len(hit), "hit", int(hit.sum()), "escape", int((~hit).sum()))
        assert 3 * hit.sum() >= len(hit) and 3 * (~hit).sum() >= len(hit)
    if name == "white_room":      # closed: every direction hits, every path runs to the budget
        assert (first_q == BOUNCES[name]).all()
    print(name, "fast" if fast else "default", "most queries of a path", int(first_q.max()), "probes differing c=0 / c=2", differ)
    for chunk in (0, 2, 1):
        check(f.scene.probes(POINTS[name], samples=S, sample_chunk=chunk, **kw), paths, chunk, (name, fast, chunk))
    check(f.scene.probes(POINTS[name], samples=1, **kw), one, 0, (name, fast, "S = 1"))
    # 65 items: a wave and one
    for chunk in (0, 16):
        check(f.scene.probes(POINTS[name][1:2], samples=65, sample_chunk=chunk, index_base=1, **kw), lone, chunk, (name, fast, "S = 65", chunk))
    assert {family(n_).info["compact"] for n_ in POINTS} == {0, 1}   # a scene of each record format


# ------------------------------------------------------------------------------------------------------ every strategy

def strategies():
    d, s = test_gpu_direct.family("room"), test_gpu_sky.family("room", "gradient")
    m, t = test_gpu_mesh_lights.family("room"), test_gpu_tree_lights.family("room")
    return {
        "lamps": (d, "direct", list(d.lists["eight"]), None),
        "sky": (s, "sky", [SKY], None),
        "lamps_sky": (s, "sky", list(s.lists["two"]) + [SKY], None),
        "area_group": (m, "mesh", list(m.lists["two"]), m.mesh),
        "area_group_sky": (m, "mesh", [SKY], m.mesh),
        "tree_group": (t, "tree", list(t.lists["two"]) + [SKY], t.mesh),
        "tree_group_alone": (t, "tree", [], t.mesh),
    }


@pytest.mark.parametrize("which", ["lamps", "sky", "lamps_sky", "area_group", "area_group_sky", "tree_group", "tree_group_alone"])
def test_every_lighting_is_its_readings(which):
    f, kind, lights, mesh = strategies()[which]
    for fast in (False, True):
        paths = _probes.lit_paths(f.readings[fast], kind, ROOM_POINTS, S, 50, SEED, lights)
        unlit = _probes.unlit_paths(f.readings[fast].osc, ROOM_POINTS, S, 50, SEED, traversal=2 if fast else 0)
        assert paths[1].max() >= 4, which
        assert (bits(_probes.answers(*paths, 0)[0]) != bits(_probes.answers(*unlit, 0)[0])).any(), which
        for chunk in (0, 2):
            got = f.scene.probes(ROOM_POINTS, samples=S, max_bounces=50, seed=SEED, sample_chunk=chunk, fast_traversal=fast, queries=True,
                                 lights=lights, direct=True, mesh=mesh)
            check(got, paths, chunk, (which, fast, chunk))


def test_an_empty_list_and_an_empty_group_give_the_unlit_bits():
    f = test_gpu_mesh_lights.family("room")
    unlit = _probes.unlit_paths(f.readings[False].osc, ROOM_POINTS, S, 50, SEED)
    kw = dict(samples=S, max_bounces=50, seed=SEED, sample_chunk=2, queries=True)
    want = check(f.scene.probes(ROOM_POINTS, **kw), unlit, 2, "lights=None")
    empty, empty_tree = f.scene.mesh_lights([]), f.scene.mesh_lights([], tree=True)
    for extra in (dict(lights=[]), dict(lights=[], direct=True), dict(lights=[], direct=True, mesh=empty),
                  dict(lights=[], direct=True, mesh=empty_tree), dict(direct=True)):
        got = f.scene.probes(ROOM_POINTS, **kw, **extra)
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1]), extra
    empty.close(), empty_tree.close()


# ------------------------------------------------------------------------------------------------------ edges

def test_no_probe_one_probe_and_a_wave_and_one():
    f = family("material_test")
    kw = dict(max_bounces=50, seed=SEED, queries=True)
    coeffs, cnt = f.scene.probes(np.zeros((0, 3)), samples=4, **kw)
    assert coeffs.shape == (0, 9, 3) and cnt.shape == (0,) and coeffs.dtype == np.float64 and cnt.dtype == np.uint32
    assert f.scene.probes(np.zeros((0, 3)), samples=4).shape == (0, 9, 3)
    check(f.scene.probes(POINTS["material_test"][:1], samples=S, sample_chunk=2, **kw), expected("material_test", n=1), 2, "n = 1")
    # 65 probes of one sample: a wave and one item, every probe a chunk of its own
    rng = np.random.default_rng(65)
    pts = np.array((0.0, 1.5, 1.0)) + rng.uniform(-1.0, 1.0, size=(65, 3)) * (6.0, 1.0, 2.0)
    paths = _probes.unlit_paths(f.osc, pts, 1, 50, SEED, 7)
    check(f.scene.probes(pts, samples=1, index_base=7, **kw), paths, 0, "n = 65, S = 1")
    only = f.scene.probes(pts, samples=1, index_base=7, max_bounces=50, seed=SEED)
    assert np.array_equal(bits(only), bits(_probes.answers(*paths, 0)[0]))


def test_one_bounce_no_bounce_and_a_probe_inside_a_sphere():
    f = family("white_room")
    pts = POINTS["white_room"]
    for bounces in (1, 2):
        paths = expected("white_room", max_bounces=bounces)
        assert (paths[1] == bounces).all()
        check(f.scene.probes(pts, samples=S, max_bounces=bounces, seed=SEED, sample_chunk=2, queries=True), paths, 2, ("max_bounces", bounces))
    coeffs, cnt = f.scene.probes(pts, samples=S, max_bounces=0, seed=SEED, queries=True)
    assert (bits(coeffs) == 0).all() and (cnt == 0).all()     # +0 and no query
    # the third probe is the centre of the glass sphere: every first ray meets the sphere from inside, at t = its radius
    w = expected("white_room")[2]
    for s in range(S):
        obj, t = f.osc.intersect(pts[2], w[2, s], f.z_near, Z_FAR)
        assert obj == 6 and abs(t - 0.8) < 1e-12, (obj, t)


def test_points_with_nan_and_infinite_components():
    """A NaN or infinite component makes no ray worth the name; the answer is NaN or what the reading gives, never a fault, and
    the probes beside it are untouched."""
    f = family("material_test")
    good = POINTS["material_test"]
    pts = np.array([good[0], (np.nan, 1.0, 1.0), good[1], (0.0, np.inf, 0.0), (1.0, 2.0, -np.inf), (np.nan, np.nan, np.nan), good[2],
                    (np.inf, -np.inf, 1e300)])
    paths = _probes.unlit_paths(f.osc, pts, S, 50, SEED)
    got = f.scene.probes(pts, samples=S, max_bounces=50, seed=SEED, sample_chunk=2, queries=True)
    want = check(got, paths, 2, "non-finite points", finite=False)
    print("non-finite points: probes with NaN in the reading", np.isnan(want[0]).any(axis=(1, 2)).tolist(), "queries", want[1].tolist())
    for k, i in ((0, 0), (2, 1), (6, 2)):   # the finite probes, each against the call that holds it alone
        alone = f.scene.probes(good[i:i + 1], samples=S, max_bounces=50, seed=SEED, sample_chunk=2, index_base=k)
        assert np.isfinite(got[0][k]).all() and np.array_equal(bits(got[0][k]), bits(alone[0]))


# ------------------------------------------------------------------------------------------------------ slices, launches

def test_a_call_on_a_slice_is_the_slice_of_the_whole_call():
    f = family("mesh3_light")
    rng = np.random.default_rng(4)
    pts = np.array((0.0, 1.5, 0.0)) + rng.uniform(-1.0, 1.0, size=(9, 3)) * (3.0, 1.2, 3.0)
    kw = dict(samples=6, max_bounces=50, seed=SEED, sample_chunk=4, queries=True)
    whole = f.scene.probes(pts, index_base=100, **kw)
    assert (whole[1] >= 6).all() and np.isfinite(whole[0]).all() and (whole[0][:, 0] > 0.0).any()
    for a, b in ((0, 9), (0, 1), (3, 7), (8, 9)):
        part = f.scene.probes(pts[a:b], index_base=100 + a, **kw)
        assert np.array_equal(bits(part[0]), bits(whole[0][a:b])) and np.array_equal(part[1], whole[1][a:b]), (a, b)
    # the seed and the index base are the key: another of either is another answer
    assert not np.array_equal(bits(f.scene.probes(pts, index_base=101, **kw)[0]), bits(whole[0]))
    assert not np.array_equal(bits(f.scene.probes(pts, index_base=100, **{**kw, "seed": SEED + 1})[0]), bits(whole[0]))


def test_device_tensors_on_a_stream_give_the_host_paths_bits():
    """tests/_probes_torch_child.py, in a process of its own (torch has to be imported before the library is loaded)."""
    pytest.importorskip("torch")
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_probes_torch_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "device path ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_two_launches_and_a_probe_in_two_rounds_of_the_projection():
    """4097 probes of 256 samples are 2^20 + 256 items: a full launch and one probe.  sample_chunk = 24 makes 11 chunks a probe,
    45,056 (probe, chunk) pairs in the first launch: two rounds of the projection's 2^15 slots, and probe 2978 (pairs 32,758 to
    32,768) has chunks in both."""
    f = family("white_room")
    n, samples, chunk, bounces = 4097, 256, 24, 2
    rng = np.random.default_rng(4097)
    pts = rng.uniform(-1.0, 1.0, size=(n, 3)) * (1.9, 1.9, 2.9)
    kw = dict(samples=samples, max_bounces=bounces, seed=SEED, sample_chunk=chunk, queries=True)
    whole = f.scene.probes(pts, **kw)
    cut = 2500
    head, tail = f.scene.probes(pts[:cut], **kw), f.scene.probes(pts[cut:], index_base=cut, **kw)
    assert np.array_equal(bits(whole[0]), bits(np.concatenate([head[0], tail[0]])))
    assert np.array_equal(whole[1], np.concatenate([head[1], tail[1]]))
    assert int(whole[1].astype(np.int64).sum()) == int(head[1].astype(np.int64).sum()) + int(tail[1].astype(np.int64).sum())
    assert whole[1].max() == samples * bounces and np.isfinite(whole[0]).all() and len(np.unique(bits(whole[0][:, 1, 0]))) > n // 4
    for i in (0, 1, 2047, 2977, 2978, 2979, 4095, 4096):
        paths = _probes.unlit_paths(f.osc, pts[i:i + 1], samples, bounces, SEED, i)
        check((whole[0][i:i + 1], whole[1][i:i + 1]), paths, chunk, ("probe", i))


# ------------------------------------------------------------------------------------------------------ neighbours

def test_the_neighbours_on_the_shared_scratch_keep_their_bits():
    f = family("material_test")
    p = np.array([(x, 0.0, z) for z in np.linspace(-3.0, 3.0, 9) for x in np.linspace(-6.0, 6.0, 9)])
    nrm = np.tile((0.0, 1.0, 0.0), (len(p), 1))
    rad_kw = dict(samples=5, sample_chunk=2, seed=SEED, queries=True)

    def neighbours():
        return f.scene.radiance(f.o, f.d, **rad_kw), f.scene.irradiance(p, nrm, bias=1e-4, **rad_kw)
    before = neighbours()
    probes = f.scene.probes(POINTS["material_test"], samples=S, seed=SEED, sample_chunk=2, queries=True)
    after = neighbours()
    again = f.scene.probes(POINTS["material_test"], samples=S, seed=SEED, sample_chunk=2, queries=True)
    for b, a in zip(before, after):
        assert np.array_equal(bits(b[0]), bits(a[0])) and np.array_equal(b[1], a[1])
    assert np.array_equal(bits(probes[0]), bits(again[0])) and np.array_equal(probes[1], again[1])
    check(again, expected("material_test"), 2, "after the neighbours")
