"""Lightmap atlases (include/rayrs_hip.h LIGHTMAP ATLAS) without a GPU: the header states the operation and the six entry points
are declared, exported and bound; the two forms of the plain-Python reading (tests/_lightmap.py) agree bit for bit on the small
cases, so that the GPU tests may use the vectorised one at size; the reading's positions lie in their triangles' planes and its
barycentrics are not negative; unwrap_triangles is deterministic, of the documented size, gives every triangle texels and keeps
the triangles' texels apart; every refusal that is decided before the device is touched comes in the header's order; the
wrappers' ValueErrors; and the new unit's kernels use no scratch memory."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _lightmap as R
import rayrs_amd
from rayrs_amd import _ffi
from rayrs_amd.api import Emission, Material, Object
from test_features import HIPCC, compile_asm, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["rayrs_lightmap_create", "rayrs_lightmap_destroy", "rayrs_lightmap_count", "rayrs_lightmap_texels", "rayrs_lightmap_owner",
                "rayrs_lightmap_assemble"]
INVALID_ARG, NO_DEVICE = -1, -4
CASES = R.cases()


def header():
    return open(os.path.join(ROOT, "include", "rayrs_hip.h")).read()


def test_the_header_states_the_operation_and_the_entry_points_are_exported_and_bound():
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(rf"\b(int|void) {name}\s*\(", code), name
    text = re.sub(r"\s+", " ", re.sub(r"\s*\n \*\s*", " ", header()))
    assert "LIGHTMAP ATLAS, specified to the operation" in text
    assert text.index("SH PROBES, specified") < text.index("LIGHTMAP ATLAS, specified")
    for phrase in ("w0(px, py) = (U2 - U1) * (py - V1) - (V2 - V1) * (px - U1)", "w1(px, py) = (U0 - U2) * (py - V2) - (V0 - V2) * (px - U2)",
                   "w2(px, py) = (U1 - U0) * (py - V0) - (V1 - V0) * (px - U0)", "b0 = (1.0 - b1) - b2", "position = (b0 * P0 + b1 * P1) + b2 * P2",
                   "the LOWEST k that covers it", "value = s / (double)count", "Refusals, in this order", "Out of scope"):
        assert phrase in text, phrase
    L = _ffi.lib()
    assert L.rayrs_abi_version() == _ffi.ABI_VERSION == 7
    for name in ENTRY_POINTS:
        assert name in _ffi.SYMBOLS and hasattr(L, name) and getattr(L, name).argtypes, name
    assert L.rayrs_lightmap_create.argtypes[-1] == C.POINTER(C.c_void_p) and L.rayrs_lightmap_destroy.restype is None
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRY_POINTS:
        assert re.search(rf"fn {name}\(", integration), name
    for name in ("Lightmap", "unwrap_triangles"):
        assert name in rayrs_amd.__all__ and callable(getattr(rayrs_amd, name)), name
    for name in ("texels", "bary", "owner", "image", "bake", "close", "from_object"):
        assert callable(getattr(rayrs_amd.Lightmap, name)), name
    assert isinstance(rayrs_amd.Lightmap.coverage, property)


# ---- the reading's two forms

@pytest.mark.parametrize("name", sorted(CASES))
def test_the_scalar_and_the_vectorised_reading_agree_bit_for_bit(name):
    verts, idx, uvs, W, H, flip = CASES[name]
    a, b = R.atlas_scalar(verts, idx, uvs, W, H, flip), R.atlas_vector(verts, idx, uvs, W, H, flip)
    assert a[0].dtype == b[0].dtype == np.uint32 and np.array_equal(a[0], b[0])
    assert np.array_equal(a[1], b[1]) and (np.diff(a[1].astype(np.int64)) > 0).all()
    for x, y in zip(a[2:], b[2:]):
        assert x.shape == (len(a[1]), 3) and R.same(x, y)
    rng = np.random.default_rng(len(name))
    for ch in (1, 3):
        values = rng.normal(size=(len(a[1]), ch))
        if len(values) > 2:
            values[0, 0], values[1, ch - 1], values[2, 0] = np.nan, np.inf, -0.0
        for d in (0, 1, 3, max(W, H) + 2) if W * H <= 256 else (0, 2):
            (i0, v0), (i1, v1) = R.assemble_scalar(a[1], values, W, H, d), R.assemble_vector(a[1], values, W, H, d)
            assert i0.shape == (H, W, ch) and R.same(i0, i1) and np.array_equal(v0, v1), (ch, d)


def test_the_readings_cases_are_what_they_are_named_for():
    own = {name: R.owner_vector(c[2], c[3], c[4]) for name, c in CASES.items()}
    n = {name: int((o != R.NO_OWNER).sum()) for name, o in own.items()}
    print(n)
    assert n["quad"] == n["quad_rewound"] == 64 and n["full_67x35"] == 67 * 35 and n["empty"] == 0
    assert (np.diag(own["quad"]) == 0).all() and (np.diag(own["quad_rewound"]) == 0).all()    # the shared edge: the lower index
    assert set(np.unique(own["quad"])) == {0, 1}
    assert set(np.unique(own["degenerate"])) == {1, 3, 5, R.NO_OWNER}
    assert set(np.unique(own["outside"])) == {0, R.NO_OWNER} and (own["outside"][:, 0] == 0).any()
    assert 0 < n["tiny_200"] < 40                                                               # most of the 200 own nothing
    assert set(np.unique(own["overlaid"])) == {0, R.NO_OWNER} and n["overlaid"] == n["one"]
    a = R.atlas_vector(*CASES["one"][:5], False)
    f = R.atlas_vector(*CASES["flip"][:5], True)
    assert R.same(a[3], -f[3]) and R.same(a[2], f[2])
    assert not R.same(a[2], R.atlas_vector(*CASES["f32"][:5], False)[2])                  # f32 vertices are other vertices
    assert np.isnan(R.atlas_vector(*CASES["degenerate"])[3]).any()


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_readings_positions_lie_in_their_triangles_planes(name):
    """Every position satisfies its triangle's plane equation to a relative 1e-12 (of the triangle's extent from the origin), and
    b0, b1, b2 >= 0: b0 is (1 - b1) - b2, not an edge function, and the cases keep it from rounding below zero."""
    verts, idx, uvs, W, H, flip = CASES[name]
    own, index, points, nrm, bary = R.atlas_vector(verts, idx, uvs, W, H, flip)
    assert (bary >= 0.0).all(), bary.min()
    if len(index) == 0:
        return
    v = R.widen(verts)
    k = own.reshape(-1)[index].astype(np.int64)
    p0 = v[np.asarray(idx, dtype=np.int64)[k, 0]]
    good = np.isfinite(nrm).all(axis=1)
    scale = np.abs(v[np.asarray(idx, dtype=np.int64)[k]]).max(axis=(1, 2))
    dist = np.abs(((points - p0) * nrm).sum(axis=1))
    print(name, "largest distance from the plane over the extent:", (dist[good] / scale[good]).max())
    assert (dist[good] <= 1e-12 * scale[good]).all()
    assert np.abs(bary.sum(axis=1) - 1.0).max() <= 4e-16


# ---- the per-triangle unwrap

@pytest.mark.parametrize("m", [1, 2, 3, 7, 320])
def test_unwrap_triangles_gives_every_triangle_texels_and_keeps_them_apart(m):
    uvs, W, H = rayrs_amd.unwrap_triangles(m, cell=8, gutter=1)
    again = rayrs_amd.unwrap_triangles(m, 8, 1)
    assert uvs.shape == (m, 3, 2) and uvs.dtype == np.float64 and np.array_equal(R.bits(uvs), R.bits(again[0])) and again[1:] == (W, H)
    cells = (m + 1) // 2
    cols = int(np.ceil(np.sqrt(cells)))
    assert (W, H) == (cols * 8, -(-cells // cols) * 8) and (cols - 1) ** 2 < cells <= cols * cols      # a near-square grid of cells
    own = R.owner_scalar(uvs, W, H) if m <= 7 else R.owner_vector(uvs, W, H)
    owned = own != R.NO_OWNER
    assert sorted(np.unique(own[owned])) == list(range(m))                                              # every triangle owns a texel
    pad = np.pad(own.astype(np.int64), 1, constant_values=R.NO_OWNER)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            nb = pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
            assert not (owned & (nb != R.NO_OWNER) & (nb != own)).any(), (dy, dx)                     # no other triangle's texel beside it
    if m % 2:                                                                                           # the last cell is half empty
        last = cells - 1
        cell = own[(last // cols) * 8:(last // cols) * 8 + 8, (last % cols) * 8:(last % cols) * 8 + 8]
        assert set(np.unique(cell)) == {m - 1, R.NO_OWNER}
    # a triangle's texels lie in its own cell
    ys, xs = np.nonzero(owned)
    assert np.array_equal(own[ys, xs] // 2, (ys // 8) * cols + xs // 8)


def test_unwrap_triangles_other_cells_gutters_and_refusals():
    for cell, gutter in ((4, 1), (6, 2), (8, 0), (16, 3)):
        uvs, W, H = rayrs_amd.unwrap_triangles(10, cell, gutter)
        own = R.owner_vector(uvs, W, H).astype(np.int64)
        owned = own != R.NO_OWNER
        assert sorted(np.unique(own[owned])) == list(range(10)), (cell, gutter)
        pad = np.pad(own, gutter, constant_values=R.NO_OWNER) if gutter else own
        for dy in range(-gutter, gutter + 1):
            for dx in range(-gutter, gutter + 1):
                nb = pad[gutter + dy:gutter + dy + H, gutter + dx:gutter + dx + W]
                assert not (owned & (nb != R.NO_OWNER) & (nb != own)).any(), (cell, gutter, dy, dx)
    assert rayrs_amd.unwrap_triangles(0)[0].shape == (0, 3, 2) and rayrs_amd.unwrap_triangles(0)[1:] == (8, 8)
    for bad in ((-1, 8, 1), (4, 3, 1), (4, 8, -1), (4, 5, 2), (2 * 2049 * 2049, 8, 1)):
        with pytest.raises(ValueError):
            rayrs_amd.unwrap_triangles(*bad)


# ---- refusals, in the header's order

def test_the_refusals_without_a_device_come_in_the_headers_order():
    L = _ffi.lib()
    verts, idx, uvs = np.zeros((3, 3)), np.array([[0, 1, 2]], dtype=np.uint32), np.zeros((1, 3, 2))
    P = lambda a: a.ctypes.data

    def create(device=-1, verts_=P(verts), f32=0, nv=3, idx_=P(idx), m=1, uvs_=P(uvs), w=8, h=8, flip=0, out=True):
        handle = C.c_void_p()
        st = L.rayrs_lightmap_create(device, verts_, f32, nv, idx_, m, uvs_, w, h, flip, C.byref(handle) if out else None)
        assert handle.value is None
        return st

    bad_idx = np.array([[0, 1, 3]], dtype=np.uint32)
    invalid = (dict(out=False), dict(verts_=None), dict(idx_=None), dict(uvs_=None), dict(f32=2), dict(flip=2), dict(w=0), dict(h=0),
               dict(w=16385), dict(h=16385), dict(idx_=P(bad_idx)), dict(nv=2))
    for bad in invalid:
        for device in (-1, 0, 1 << 20):   # RAYRS_INVALID_ARG stands before RAYRS_NO_DEVICE whatever the device
            assert create(device=device, **bad) == INVALID_ARG, bad
    # within the group: the earlier refusal is not undone by a later one
    assert create(verts_=None, w=0, idx_=P(bad_idx)) == INVALID_ARG
    for ok in (dict(), dict(f32=1), dict(flip=1), dict(w=16384, h=16384), dict(m=0, verts_=None, idx_=None, uvs_=None, nv=0), dict(m=0)):
        assert create(**ok) == NO_DEVICE, ok
        assert create(device=1 << 20, **ok) == NO_DEVICE, ok
    n, out = C.c_uint64(7), np.zeros(64)
    assert L.rayrs_lightmap_count(None, C.byref(n)) == INVALID_ARG and n.value == 7
    assert L.rayrs_lightmap_texels(None, None, None, None, None) == INVALID_ARG
    assert L.rayrs_lightmap_owner(None, P(out)) == INVALID_ARG
    assert L.rayrs_lightmap_assemble(None, P(out), 1, 0, P(out), None) == INVALID_ARG
    L.rayrs_lightmap_destroy(None)


def test_the_wrappers_value_errors():
    verts, idx, uvs = np.zeros((4, 3)), np.array([[0, 1, 2], [0, 2, 3]]), np.zeros((2, 3, 2))
    for bad in (dict(verts=np.zeros((4, 2))), dict(idx=np.array([0, 1, 2])), dict(idx=np.array([[0, 1, 4]])), dict(idx=np.array([[0, -1, 2]])),
                dict(idx=np.array([[0.0, 1.0, 2.0]])), dict(uvs=np.zeros((2, 3))), dict(uvs=np.zeros((3, 2))), dict(uvs=np.zeros((2, 3, 3))),
                dict(width=0), dict(height=0), dict(width=16385), dict(height=1 << 20)):
        args = dict(verts=verts, idx=idx, uvs=uvs, width=8, height=8)
        args.update(bad)
        with pytest.raises(ValueError):
            rayrs_amd.Lightmap(device=-1, **args)
    # what is legal reaches the library, which has no such device: per-corner and per-vertex uvs, f32 vertices, no triangle
    for args in ((verts, idx, uvs, 8, 8), (verts, idx, np.zeros((4, 2)), 8, 8), (verts.astype(np.float32), idx, uvs, 16384, 1),
                 (np.zeros((0, 3)), np.zeros((0, 3), dtype=np.uint32), np.zeros((0, 3, 2)), 4, 4)):
        with pytest.raises(_ffi.RayrsError) as e:
            rayrs_amd.Lightmap(*args, flip=True, device=-1)
        assert e.value.status == NO_DEVICE
    mesh = Object.from_triangles(verts, idx, Material.NoReflect(), Emission.Dark())
    with pytest.raises(_ffi.RayrsError) as e:
        rayrs_amd.Lightmap.from_object(mesh, device=-1)          # the one-element list from_triangles returns
    assert e.value.status == NO_DEVICE
    with pytest.raises(_ffi.RayrsError):
        rayrs_amd.Lightmap.from_object(mesh[0], cell=4, device=-1)
    for bad in (dict(obj=Object.sphere(1.0, (0, 0, 0), Material.NoReflect(), Emission.Dark())), dict(uvs=uvs), dict(uvs=uvs, width=8),
                dict(cell=3), dict(width=9), dict(height=9)):
        args = dict(obj=mesh[0], device=-1)
        args.update(bad)
        with pytest.raises(ValueError):
            rayrs_amd.Lightmap.from_object(**args)


# ---- kernel resources

@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_the_lightmap_kernels_use_no_scratch_and_no_lds_beyond_the_scans(tmp_path):
    res = kernel_resources(compile_asm("lightmap.hip", tmp_path))
    # owner, owner_big, count, scan, record, scatter, and the dilation for 1 .. 4 channels
    assert len(res) == 10 and sum("lightmap_dilate_kernel" in n for n in res) == 4
    for name, (vgpr, scratch, lds) in sorted(res.items()):
        print(name, vgpr, scratch, lds)
        want_lds = 64 if "scan" in name else 16 if ("count" in name or "record" in name) else 0      # the wave totals, 4 bytes each
        assert scratch == 0 and lds == want_lds and vgpr <= 128, (name, vgpr, scratch, lds)
