"""Lightmap atlases (include/rayrs_hip.h LIGHTMAP ATLAS) on the GPU, bit for bit against the plain-Python reading
(tests/_lightmap.py): the owner plane, the texel list in its order, the positions, the normals and the barycentrics on the small
cases (the scalar reading) and on two large ones (the vectorised reading, which tests/test_lightmap.py holds equal to the scalar
one); the assembly with NaN, +inf and -0.0 among the values; two atlases alive at once; and the whole job on the level-1 mesh
scene, where a bake made through the atlas is the Bake's own contract -- scene.irradiance of the same points -- and its image the
reading's assembly of those values.  A NaN (a normal of a triangle without area in space) is equal to any NaN."""
import functools

import numpy as np
import pytest

import _lightmap as R
import rayrs_amd
from rayrs_amd import procedural
from test_gpu_mesh_lights import mesh1_objects

pytestmark = pytest.mark.gpu

CASES = R.cases()
HDRI = procedural.make_studio_hdri(9, 5)
SEED = 0x5EED


def check_atlas(lm, want):
    own, index, points, normals, bary = want
    H, W = own.shape
    assert lm.n == len(index) and lm.coverage == len(index) / float(W * H)
    got_own = lm.owner()
    want_own = own.astype(np.int64)
    want_own[own == R.NO_OWNER] = -1
    assert got_own.dtype == np.int64 and got_own.shape == (H, W) and np.array_equal(got_own, want_own)
    i, p, n = lm.texels()
    b = lm.bary()
    assert i.dtype == np.uint32 and np.array_equal(i, index)
    for got, ref, what in ((p, points, "points"), (n, normals, "normals"), (b, bary, "bary")):
        assert got.shape == (len(index), 3) and got.dtype == np.float64 and R.same(got, ref), what
    finite = np.isfinite(normals)
    assert np.array_equal(R.bits(n[finite]), R.bits(normals[finite]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_atlas_is_the_scalar_readings(name):
    verts, idx, uvs, W, H, flip = CASES[name]
    lm = rayrs_amd.Lightmap(verts, idx, uvs, W, H, flip=flip)
    check_atlas(lm, R.atlas_scalar(verts, idx, uvs, W, H, flip))
    lm.close()
    lm.close()
    with pytest.raises(rayrs_amd._ffi.RayrsError):
        lm.texels()


def test_per_vertex_uvs_are_expanded_through_the_indices():
    verts = np.array([(0.0, 0.0, 0.0), (2.0, 0.0, 1.0), (2.0, 3.0, 1.0), (0.0, 3.0, 0.0)])
    idx = np.array([(0, 1, 2), (0, 2, 3)], dtype=np.uint32)
    uv = np.array([(0.05, 0.1), (0.95, 0.05), (0.9, 0.9), (0.1, 0.95)])
    lm = rayrs_amd.Lightmap(verts, idx, uv, 13, 9)
    check_atlas(lm, R.atlas_scalar(verts, idx, uv, 13, 9))


def test_a_1030_x_1030_atlas_covered_by_two_triangles():
    """1,060,900 owned texels: 4145 workgroup counts in the scan (five of its steps), and two triangles whose candidates are the
    whole atlas, which the owner pass hands to the whole grid."""
    verts, idx = R._space(2, 11)
    uvs = np.array([[(0.0, 0.0), (1.0, 0.0), (1.0, 1.0)], [(0.0, 0.0), (1.0, 1.0), (0.0, 1.0)]])
    want = R.atlas_vector(verts, idx, uvs, 1030, 1030)
    assert len(want[1]) == 1030 * 1030 and (np.diag(want[0]) == 0).all()
    lm = rayrs_amd.Lightmap(verts, idx, uvs, 1030, 1030)
    check_atlas(lm, want)
    values = np.random.default_rng(2).normal(size=(lm.n, 3))
    img, valid = lm.image(values, dilate=2, return_valid=True)
    assert valid.all() and np.array_equal(R.bits(img.reshape(-1, 3)), R.bits(values))


def test_more_triangles_than_the_owner_pass_has_lanes():
    """530,000 triangles, unwrapped at cell = 4: the owner pass's grid is 2048 workgroups of 256 lanes, so its waves come round
    a second time."""
    m = 530000
    rng = np.random.default_rng(12)
    verts = rng.uniform(-1.0, 1.0, size=(1000, 3)).astype(np.float32)
    idx = rng.integers(0, 1000, size=(m, 3)).astype(np.uint32)
    uvs, W, H = rayrs_amd.unwrap_triangles(m, cell=4)
    want = R.atlas_vector(verts, idx, uvs, W, H, small=4)
    assert (W, H) == (2060, 2060) and len(want[1]) == 2 * m
    lm = rayrs_amd.Lightmap(verts, idx, uvs, W, H)
    check_atlas(lm, want)


@pytest.mark.parametrize("name", ["one", "degenerate", "tiny_200", "icosphere_320", "empty"])
def test_the_assembly_is_the_readings(name):
    verts, idx, uvs, W, H, flip = CASES[name]
    lm = rayrs_amd.Lightmap(verts, idx, uvs, W, H, flip=flip)
    index = lm.texels()[0]
    rng = np.random.default_rng(len(name))
    for ch in (1, 3):
        values = rng.normal(size=(lm.n, ch))
        if lm.n > 2:
            values[0, 0], values[1, ch - 1], values[2, 0] = np.nan, np.inf, -0.0
        for d in (0, 1, 3, max(W, H) + 3):
            img, valid = lm.image(values, dilate=d, return_valid=True)
            want_img, want_valid = R.assemble_vector(index, values, W, H, d) if W * H > 256 else R.assemble_scalar(index, values, W, H, d)
            assert img.shape == (H, W, ch) and valid.dtype == bool and np.array_equal(valid, want_valid), (ch, d)
            assert R.same(img, want_img), (ch, d)
            assert np.array_equal(R.bits(img[~valid]), np.zeros((int((~valid).sum()), ch), dtype=np.uint64))   # +0 where nothing is
            if d == 0 and lm.n > 2:
                assert np.signbit(img.reshape(-1, ch)[index[2], 0]) and np.isnan(img.reshape(-1, ch)[index[0], 0])
            if d > max(W, H) and lm.n > 0:
                assert valid.all()
    flat = lm.image(np.arange(lm.n, dtype=np.float64), dilate=0)
    assert flat.shape == (H, W) and np.array_equal(flat.reshape(-1)[index], np.arange(lm.n))
    for bad in (np.zeros((lm.n + 1, 3)), np.zeros((lm.n, 5)), np.zeros((lm.n, 2, 2))):
        with pytest.raises(ValueError):
            lm.image(bad)
    with pytest.raises(ValueError):
        lm.image(np.zeros(lm.n), dilate=-1)


def test_two_atlases_alive_at_once_leave_each_other_alone():
    a_case, b_case = CASES["icosphere_320"], CASES["degenerate"]
    a = rayrs_amd.Lightmap(*a_case[:5], flip=a_case[5])
    b = rayrs_amd.Lightmap(*b_case[:5], flip=b_case[5])
    want_a, want_b = R.atlas_scalar(*a_case), R.atlas_scalar(*b_case)
    va, vb = np.random.default_rng(1).normal(size=(a.n, 3)), np.random.default_rng(2).normal(size=(b.n, 1))
    img_a = a.image(va, dilate=2)
    img_b = b.image(vb, dilate=5)
    check_atlas(a, want_a)
    assert R.same(a.image(va, dilate=2), img_a) and R.same(img_a, R.assemble_vector(want_a[1], va, a_case[3], a_case[4], 2)[0])
    b.close()
    check_atlas(a, want_a)
    b = rayrs_amd.Lightmap(*b_case[:5], flip=b_case[5])
    a.close()
    check_atlas(b, want_b)
    assert R.same(b.image(vb, dilate=5), img_b) and R.same(img_b, R.assemble_scalar(want_b[1], vb, b_case[3], b_case[4], 5)[0])


# ---- the whole job

@functools.lru_cache(maxsize=None)
def mesh1():
    _, objs, heur, _ = mesh1_objects()
    scene = rayrs_amd.Scene(objs, 1e-6, 1e6, heur, HDRI, device=0)
    lm = rayrs_amd.Lightmap.from_object(objs[1], cell=8)
    return objs, scene, lm


def test_the_atlas_of_the_level_1_mesh_is_the_readings_and_its_normals_are_the_scenes():
    objs, scene, lm = mesh1()
    mesh = objs[1]
    uvs, W, H = rayrs_amd.unwrap_triangles(len(mesh.idx), 8, 1)
    assert (lm.width, lm.height, lm.m) == (W, H, 80) and mesh.verts.dtype == np.float32
    want = R.atlas_scalar(mesh.verts, mesh.idx, uvs, W, H)
    check_atlas(lm, want)
    # the normal of a texel is the bits scene.intersect reports for a hit on its triangle: a ray down the normal onto the texel
    index, points, normals = lm.texels()
    t, obj, n_hit = scene.intersect(points + normals * 1e-3, -normals, normals=True)
    owner = lm.owner().reshape(-1)[index]
    hit_own = obj == 1 + owner                                   # (the mesh's triangles are objects 1 .. 80)
    assert hit_own.mean() > 0.9
    assert np.array_equal(R.bits(n_hit[hit_own]), R.bits(normals[hit_own]))


@pytest.mark.parametrize("lit", [False, True])
def test_a_bake_through_the_atlas_is_the_bakes_contract_and_its_image_the_readings(lit):
    objs, scene, lm = mesh1()
    index, points, normals = lm.texels()
    lighting = dict(lights=rayrs_amd.emitters(objs), direct=True) if lit else {}
    bake = lm.bake(scene, sample_chunk=4, seed=SEED, bias=1e-4, **lighting)
    assert bake.kind == "irradiance" and bake.n == lm.n
    bake.render(8)
    values, queries = bake.values(queries=True)
    want, want_queries = scene.irradiance(points, normals, samples=8, sample_chunk=4, seed=SEED, bias=1e-4, queries=True, **lighting)
    assert np.array_equal(R.bits(values), R.bits(want)) and np.array_equal(queries.astype(np.uint64), want_queries.astype(np.uint64))
    assert (values > 0.0).any() and np.isfinite(values).all()
    img, valid = lm.image(values, dilate=2, return_valid=True)
    want_img, want_valid = R.assemble_vector(index, values, lm.width, lm.height, 2)
    assert np.array_equal(R.bits(img), R.bits(want_img)) and np.array_equal(valid, want_valid) and valid.sum() > lm.n
    bake.close()
    with pytest.raises(ValueError):
        lm.bake(scene, kind="radiance")
