"""SH probes (include/rayrs_hip.h SH PROBES) without a GPU: the entry points are declared, exported and bound; the library's
directions and basis on the host are the plain-Python reading's (tests/_probes.py) bit for bit; the basis is orthonormal under the
library's own directions; sh_irradiance and sh_radiance do what they say; every refusal that is decided before the device is
touched comes in the header's order; the wrapper's ValueErrors; and the new unit's kernels keep their resources."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _probes
import rayrs_amd
from rayrs_amd import SKY, _ffi
from test_features import HIPCC, compile_asm, kernel_resources
from test_mesh_lights import refusal_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["rayrs_scene_probes", "rayrs_scene_probes_launch"]
HOST_CALLS = ["rayrs_probe_directions", "rayrs_sh_basis"]
INVALID_ARG, NO_DEVICE, UNSUPPORTED = -1, -4, -5
F = np.float64


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def header():
    return open(os.path.join(ROOT, "include", "rayrs_hip.h")).read()


def test_the_header_states_the_operation_and_the_entry_points_are_exported_and_bound():
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in ENTRY_POINTS + HOST_CALLS:
        assert re.search(rf"\bint {name}\s*\(", code), name
    text = re.sub(r"\s+", " ", re.sub(r"\s*\n \*\s*", " ", header()))
    assert "SH PROBES, specified to the operation" in text
    assert text.index("LIGHT TREE, specified") < text.index("SH PROBES, specified")
    for k in ("0.28209479177387814", "0.4886025119029199", "1.0925484305920792", "0.31539156525252005", "0.5462742152960396"):
        assert k in text
    assert "FOUR_PI * (1.0 / (double)S)" in text and "Out of scope" in text
    L = _ffi.lib()
    assert L.rayrs_abi_version() == _ffi.ABI_VERSION == 7
    for name in ENTRY_POINTS + HOST_CALLS:
        assert name in _ffi.SYMBOLS and hasattr(L, name) and getattr(L, name).argtypes, name
    mesh = L.rayrs_scene_radiance_mesh.argtypes   # (scene, origin, direction, n, ...): a probe call has one array, not two
    assert L.rayrs_scene_probes.argtypes == mesh[:2] + mesh[3:]
    assert L.rayrs_scene_probes_launch.argtypes == L.rayrs_scene_probes.argtypes + [C.c_void_p]
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRY_POINTS + HOST_CALLS:
        assert re.search(rf"fn {name}\(", integration), name
    for name in ("probe_directions", "sh_basis", "sh_radiance", "sh_irradiance", "probe_grid"):
        assert name in rayrs_amd.__all__ and callable(getattr(rayrs_amd, name)), name
    assert callable(rayrs_amd.Scene.probes)


# ---- the host calls against the reading

def test_probe_directions_are_the_readings():
    for n, samples, seed, base in ((3, 7, 0x5EED, 0), (1, 1, 0, 0), (2, 33, 2 ** 64 - 1, 2 ** 40 + 5), (0, 4, 1, 0), (2, 0, 1, 0)):
        got = rayrs_amd.probe_directions(n, samples, seed, base)
        want = _probes.directions(n, samples, seed, base)
        assert got.shape == (n, samples, 3) and got.dtype == np.float64
        assert np.array_equal(bits(got), bits(want)), (n, samples, seed, base)
    # a slice of a call is the call on the slice, and the directions lie on the unit sphere to rounding
    whole = rayrs_amd.probe_directions(9, 16, 11, 100)
    assert np.array_equal(bits(whole[3:7]), bits(rayrs_amd.probe_directions(4, 16, 11, 103)))
    assert np.abs(np.linalg.norm(whole, axis=-1) - 1.0).max() < 4e-16
    assert _ffi.lib().rayrs_probe_directions(1, 0, 1, 1, None) == INVALID_ARG


def test_the_basis_is_the_readings_with_nan_and_infinite_components_too():
    rng = np.random.default_rng(3)
    d = np.concatenate([rayrs_amd.probe_directions(4, 8, 5, 0).reshape(-1, 3), rng.normal(size=(16, 3)) * 1e3,
                        [(0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (-0.0, 0.0, 0.0), (1e308, 1e308, 1e-308), (5e-324, 1.0, 2.0)],
                        [(np.nan, 0.5, 0.5), (0.5, np.nan, 0.5), (0.5, 0.5, np.nan), (np.inf, 1.0, 1.0), (1.0, -np.inf, 2.0),
                         (1.0, 2.0, np.inf), (np.inf, np.inf, 0.0), (np.inf, 0.0, -np.inf), (0.0, np.inf, 0.0), (np.nan, np.inf, -np.inf)]])
    got = rayrs_amd.sh_basis(d)
    want = np.array([_probes.basis(w) for w in d])
    assert got.shape == (len(d), 9) and _probes.same_or_nan(got, want)
    finite = np.isfinite(d).all(axis=1)
    assert np.array_equal(bits(got[finite]), bits(want[finite]))
    assert np.array_equal(np.isnan(got), np.isnan(want)) and (~np.isfinite(got[~finite])).any(axis=1).all() and np.isnan(got).any()
    assert rayrs_amd.sh_basis(np.zeros((0, 3))).shape == (0, 9)
    L = _ffi.lib()
    out = np.zeros(9)
    assert L.rayrs_sh_basis(None, 1, out.ctypes.data) == INVALID_ARG and L.rayrs_sh_basis(out.ctypes.data, 1, None) == INVALID_ARG
    with pytest.raises(ValueError):
        rayrs_amd.sh_basis(np.zeros((2, 2)))


def test_the_basis_is_orthonormal_under_the_librarys_own_directions():
    """(4 pi / S) sum_s Y_j(w_s) Y_k(w_s) is delta_jk within 5 standard errors, the error from the samples themselves (as
    tests/test_lit.py does for its densities).  Y_0 * Y_0 is a constant, its sample error zero: what is left there is the rounding
    of a sum of S terms, S * 2^-52."""
    S = 16384
    w = rayrs_amd.probe_directions(4, S // 4, 0x5EED, 0).reshape(-1, 3)
    Y = rayrs_amd.sh_basis(w)
    worst = 0.0
    for j in range(9):
        for k in range(j, 9):
            f = 4.0 * np.pi * Y[:, j] * Y[:, k]
            mean, se = f.mean(), f.std(ddof=1) / np.sqrt(S)
            z = abs(mean - (1.0 if j == k else 0.0)) / se if se > 0 else 0.0
            worst = max(worst, z)
            assert abs(mean - (1.0 if j == k else 0.0)) <= 5.0 * se + S * 2.0 ** -52, (j, k, mean, se)
            assert (j, k) == (0, 0) or 1e-3 < se < 0.02, (j, k, se)   # (the bound binds: the errors are those of S samples)
    print("45 pairs, S =", S, "worst deviation in standard errors", worst)


# ---- evaluating the coefficients

def test_sh_irradiance_of_a_constant_radiance_is_that_radiance():
    v = np.array([0.25, 1.0, 3.5])
    coeffs = np.zeros((9, 3))
    coeffs[0] = v * np.sqrt(4.0 * np.pi)
    normals = np.concatenate([rayrs_amd.probe_directions(1, 32, 9, 0)[0], [(0.0, 0.0, 1.0), (0.0, -1.0, 0.0), (1.0, 0.0, 0.0)]])
    for fn in (rayrs_amd.sh_irradiance, rayrs_amd.sh_radiance):
        got = fn(coeffs, normals)
        assert isinstance(got, np.ndarray) and got.shape == (len(normals), 3)
        assert (np.abs(got - v) <= 4 * np.spacing(v)).all(), np.abs(got - v).max()   # (torch in, torch out: tests/_probes_torch_child.py)
    # the band factors: a pure l = 1 and a pure l = 2 field come back scaled by 2/3 and 1/4
    for k, band in ((1, 2.0 / 3.0), (3, 2.0 / 3.0), (4, 0.25), (6, 0.25), (8, 0.25)):
        c = np.zeros((9, 3))
        c[k] = (1.0, 2.0, -3.0)
        rad, irr = rayrs_amd.sh_radiance(c, normals), rayrs_amd.sh_irradiance(c, normals)
        assert np.abs(rad).max() > 0.1 and np.allclose(irr, band * rad, rtol=1e-15, atol=1e-16), k


def test_sh_radiance_reproduces_a_field_of_degree_two():
    """A radiance field that is a polynomial of degree 2 in d lies in the span of Y_0 .. Y_8 on the unit sphere: its coefficients,
    found from the library's basis at 64 directions, give the field back at 256 others to rounding; so does a batch of probes."""
    rng = np.random.default_rng(17)
    a, b, M = rng.normal(size=3), rng.normal(size=(3, 3)), rng.normal(size=(3, 3, 3))

    def field(d):
        return a + d @ b + np.einsum("ni,ijc,nj->nc", d, M, d)
    fit = rayrs_amd.probe_directions(1, 64, 1, 0)[0]
    coeffs = np.linalg.lstsq(rayrs_amd.sh_basis(fit), field(fit), rcond=None)[0]
    assert coeffs.shape == (9, 3)
    d = rayrs_amd.probe_directions(1, 256, 2, 7)[0]
    want = field(d)
    got = rayrs_amd.sh_radiance(coeffs, d)
    print("degree-2 field: largest error", np.abs(got - want).max(), "of values up to", np.abs(want).max())
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    # leading axes broadcast: 5 probes, each evaluated in its own 256 directions
    many = np.stack([coeffs * s for s in (1.0, 2.0, -1.0, 0.5, 0.0)])
    got = rayrs_amd.sh_radiance(many[:, None], d[None])
    assert got.shape == (5, 256, 3) and np.abs(got[1] - 2.0 * want).max() <= 1e-11 and (got[4] == 0.0).all()


# ---- refusals, in the header's order

@pytest.mark.parametrize("n", [4, 0])
def test_the_refusals_on_a_host_only_scene_come_in_the_headers_order(n):
    L = _ffi.lib()
    scene, other, black = refusal_scene(), refusal_scene(), refusal_scene(np.zeros((5, 9, 3), dtype=np.float32))
    mesh, tree, empty, foreign, on_black = (scene.mesh_lights([6, 11]), scene.mesh_lights([6, 11], tree=True), scene.mesh_lights([]),
                                            other.mesh_lights([6]), black.mesh_lights([6]))
    x, coeffs, cnt = np.zeros((4, 3)), np.zeros((4, 9, 3)), np.zeros(4, dtype=np.uint32)
    P = lambda v: v.ctypes.data
    u32 = lambda *v: np.array(v, dtype=np.uint32)
    good = u32(3, 4, 5)

    def call(launch, sc=scene, m=mesh, sky=0, x_=P(x), samples=4, bounces=50, chunk=0, fast=0, lights=good, n_lights=None, coeffs_=P(coeffs),
             cnt_=P(cnt), no_scene=False):
        lp = None if lights is None else P(lights)
        nl = (0 if lights is None else len(lights)) if n_lights is None else n_lights
        args = (None if no_scene else sc._h, x_, n, samples, bounces, chunk, 1, 0, fast, lp, nl, None if m is None else m._h, sky, coeffs_, cnt_)
        return L.rayrs_scene_probes_launch(*args, None) if launch else L.rayrs_scene_probes(*args)

    for launch in (False, True):
        for m in (mesh, tree, empty, None):
            for bad in (dict(no_scene=True), dict(x_=None), dict(coeffs_=None), dict(samples=0), dict(fast=2), dict(sky=2),
                        dict(lights=None, n_lights=3), dict(lights=u32(3, 100)), dict(lights=u32(0xffffffff))):
                assert call(launch, m=m, **bad) == INVALID_ARG, (launch, bad)
                if "samples" not in bad:   # the RAYRS_INVALID_ARG group stands before all of the RAYRS_UNSUPPORTED group
                    assert call(launch, m=m, bounces=8001, **bad) == INVALID_ARG
                    assert call(launch, m=m, samples=(1 << 20) + 1, **bad) == INVALID_ARG
                    assert call(launch, m=m, lights=u32(6), **{k: v for k, v in bad.items() if k not in ("lights", "n_lights")}) == \
                        (INVALID_ARG if "lights" not in bad else UNSUPPORTED)
            for big in (dict(samples=(1 << 20) + 1), dict(samples=1 << 30), dict(bounces=8001), dict(samples=1 << 20, bounces=2048),
                        dict(lights=u32(3, 4, 5, 3, 4, 5, 3, 4, 5)), dict(lights=u32(3, 6)), dict(lights=u32(6))):
                assert call(launch, m=m, **big) == UNSUPPORTED, (launch, big)
            for ok in (dict(), dict(fast=1), dict(sky=1), dict(cnt_=None), dict(bounces=0), dict(lights=None), dict(chunk=1),
                       dict(lights=u32(3, 3, 3, 3, 4, 4, 4, 4)), dict(samples=1 << 20, chunk=1, bounces=2047)):
                assert call(launch, m=m, **ok) == NO_DEVICE, (launch, ok)
        # a group of another scene: RAYRS_INVALID_ARG, before everything of the RAYRS_UNSUPPORTED group
        for extra in (dict(), dict(bounces=8001), dict(lights=u32(6)), dict(sky=1), dict(samples=(1 << 20) + 1)):
            assert call(launch, m=foreign, **extra) == INVALID_ARG, extra
        # SKY SAMPLING's empty table, with sky = 1 only, after the rest of the RAYRS_UNSUPPORTED group
        assert call(launch, sc=black, m=on_black, sky=0) == NO_DEVICE
        assert call(launch, sc=black, m=on_black, sky=1) == UNSUPPORTED
        assert call(launch, sc=black, m=None, sky=1) == UNSUPPORTED
        assert call(launch, sc=black, m=on_black, sky=1, samples=0) == INVALID_ARG
    for h in (mesh, tree, empty, foreign, on_black):
        h.close()


def test_the_wrappers_value_errors():
    scene = refusal_scene()
    mesh = scene.mesh_lights([6])
    x = np.zeros((2, 3))
    with pytest.raises(ValueError):
        scene.probes(x, lights=[3])                 # a list without direct=True: the one-sample mix has no probes
    with pytest.raises(ValueError):
        scene.probes(x, lights=[SKY])
    with pytest.raises(ValueError):
        scene.probes(x, mesh=mesh)                  # a group without direct=True
    with pytest.raises(ValueError):
        scene.probes(x, lights=[3], mesh=mesh)
    with pytest.raises(ValueError):
        scene.probes(np.zeros((2, 2)))
    with pytest.raises(ValueError):
        scene.probes(x, samples=0)
    # what is legal reaches the library, which has no device here: lights=None, lights=[] and direct=True with either
    for kw in (dict(), dict(lights=None), dict(lights=[]), dict(lights=[], direct=True), dict(lights=[3], direct=True),
               dict(lights=[3, SKY], direct=True, mesh=mesh), dict(direct=True)):
        with pytest.raises(_ffi.RayrsError) as e:
            scene.probes(x, samples=4, **kw)
        assert e.value.status == NO_DEVICE, kw
    with pytest.raises(ValueError):
        rayrs_amd.probe_grid(scene, (2, 0, 2))
    mesh.close()


def test_probe_grid_is_the_cell_centres_of_the_root_box():
    scene = refusal_scene()
    b = np.array(scene.info()["root_box"])
    if np.isfinite(b).all():
        g = rayrs_amd.probe_grid(scene, (4, 2, 3))
        assert g.shape == (24, 3) and g.dtype == np.float64 and g.flags["C_CONTIGUOUS"]
        lo, hi = b[0::2], b[1::2]
        assert (g > lo).all() and (g < hi).all()
        assert np.allclose(g[0], lo + (hi - lo) / np.array([8.0, 4.0, 6.0])) and np.allclose(g[-1], hi - (hi - lo) / np.array([8.0, 4.0, 6.0]))
        assert np.allclose(g[1] - g[0], ((hi[0] - lo[0]) / 4.0, 0.0, 0.0))          # x runs fastest
        assert np.allclose(g.mean(axis=0), (lo + hi) / 2.0)
    else:
        with pytest.raises(ValueError):
            rayrs_amd.probe_grid(scene, (4, 2, 3))


# ---- kernel resources: what the other waves' units are held to
VGPR_BOUND = 256


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_the_probe_kernels_use_no_scratch_and_keep_two_waves_per_simd(tmp_path):
    res = kernel_resources(compile_asm("radiance_probe.hip", tmp_path))
    waves = {n: r for n, r in res.items() if re.search(r"probe_(direct|sky|mesh|tree)_kernel", n)}
    projection = {n: r for n, r in res.items() if "probe_project_kernel" in n or "probe_gather_kernel" in n}
    # COMPACT x EXACT of the direct and the sky wave, COMPACT x EXACT x SKY of the mesh and the tree wave; the projection's two
    assert len(waves) == 24 and len(projection) == 2 and len(res) == 26
    for name, (vgpr, scratch, lds) in sorted(res.items()):
        print(name, vgpr, scratch, lds)
        assert vgpr <= VGPR_BOUND and scratch == 0 and lds == 0, (name, vgpr, scratch, lds)   # (the stacks are dynamic LDS)
    print("wave instances:", min(v for v, _, _ in waves.values()), "to", max(v for v, _, _ in waves.values()), "VGPRs; projection:",
          sorted(v for v, _, _ in projection.values()))
