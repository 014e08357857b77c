"""The non-finite corners of the radiance half of the path, on the CPU: the scene families of _nonfinite.py show what
they claim on the oracle (so no GPU case can quietly lose its edge), the oracle's materials at those edges land on the
second reading of material.rs, the oracle's background of odd-shaped HDRIs with NaN, infinite, negative, huge and
subnormal texels lands on the second reading of lib.rs, and f32-subnormal coordinates keep the compact layout."""
import contextlib
import types

import numpy as np
import pytest

import _nonfinite as N
import _oracle
import rayrs_amd
import test_second_reading_of_lib_rs as L2
import test_second_reading_of_material_rs as M2


def oracle_frame(desc, spp=N.SPP, chunk=0):
    cam_args, objs, heur, hdri = desc
    osc = _oracle.OracleScene(objs, 1e-6, 1e6, heur, hdri)
    ocam = _oracle.OracleCamera(*cam_args)
    ref, st = osc.render(ocam, spp, N.BUDGET, sample_chunk=chunk)
    return osc, ocam, ref, st


def nan_paths_pass_the_roulette(osc, ocam, ref):
    """Traces of the samples of NaN pixels: does a path whose throughput is NaN after a bounce go on to the next one
    (p = rr_max of three NaN components is NaN, and `random > NaN` is false)?"""
    px = np.argwhere(np.isnan(ref).any(axis=2))[:24]
    pix = [(int(r), int(c)) for r, c in px for _ in range(N.SPP)]
    sam = [s for _ in px for s in range(N.SPP)]
    tr = osc.path_traces(ocam, pix, sam, 0x5EED, N.BUDGET, cap=N.BUDGET)
    for k in range(len(pix)):
        n = int(tr["n"][k])
        nan_at = np.flatnonzero(np.isnan(tr["thr"][k, :n]).all(axis=1))
        if len(nan_at) and tr["obj"][k, nan_at[0]] >= 0 and nan_at[0] + 1 < n and tr["obj"][k, nan_at[0] + 1] >= 0:
            return True
    return False


def partly_nan_paths_go_on(osc, ocam, ref):
    """Traces of the samples of NaN pixels: is a path's throughput NaN in some components only, with a surface hit
    after it (where rr_max's NaN rule decides the roulette)?"""
    px = np.argwhere(np.isnan(ref).any(axis=2))[:64]
    pix = [(int(r), int(c)) for r, c in px for _ in range(N.SPP)]
    sam = [s for _ in px for s in range(N.SPP)]
    tr = osc.path_traces(ocam, pix, sam, 0x5EED, N.BUDGET, cap=N.BUDGET)
    for k in range(len(pix)):
        n = int(tr["n"][k])
        nan = np.isnan(tr["thr"][k, :n])
        at = np.flatnonzero(nan.any(axis=1) & ~nan.all(axis=1))
        if len(at) and at[0] + 1 < n and tr["obj"][k, at[0] + 1] >= 0:
            return True
    return False


@pytest.mark.parametrize("name", list(N.FAMILIES))
def test_family_shows_its_edge_on_the_oracle(name):
    fn, claims = N.FAMILIES[name]
    osc, ocam, ref, st = oracle_frame(fn())
    assert st["paths"] == N.W * N.H * N.SPP
    nan_px = np.isnan(ref).any(axis=2)
    assert st["nan_pixels"] == int(nan_px.sum())
    f32 = ref.astype(np.float32) if "over_f32" not in claims else None
    if "nan" in claims:
        assert st["nan_pixels"] > 0
    if "nan_thr" in claims:
        assert nan_paths_pass_the_roulette(osc, ocam, ref)
    if "part_nan_thr" in claims:
        assert partly_nan_paths_go_on(osc, ocam, ref)
    if "part_nan" in claims:
        assert (nan_px & ~np.isnan(ref).all(axis=2)).any()
    if "inf" in claims:
        assert np.isinf(ref).any()
    if "over_f32" in claims:
        fin = ref[np.isfinite(ref)]
        assert (fin > N.F32_MAX).any()
        with np.errstate(over="ignore"):
            assert np.isinf(ref.astype(np.float32)[np.isfinite(ref)]).any()
    if "sub32" in claims:
        a = np.abs(f32)
        assert ((a > 0) & (a < N.F32_TINY)).sum() > 100
    if "finite" in claims:
        assert np.isfinite(ref).all() and st["nan_pixels"] == 0
    if "big_weight" in claims:
        nrm, view, key = N.edge_normals_views()
        sc, col, _, _ = _oracle.material_evaluate(fn()[1][1].mat, nrm, view, key)
        w = col[sc == 1].max(axis=1)
        assert len(w) > 1000 and (w > 1.0).mean() > 0.4


def test_nan_roulette_keeps_paths_going():
    """p = rr_max of three NaN components is NaN, `random > p` is false: the path goes on to the budget.  That is
    what raises the family's ray count above the same scene's with a finite surface."""
    _, _, _, st = oracle_frame(N.FAMILIES["ct_alpha_1e-200"][0]())
    from rayrs_amd.api import Fresnel, Material
    _, _, _, st0 = oracle_frame(N.floor_and_sphere(Material.CookTorrance(N.ONE, 0.3, Fresnel.SchlickMetallic((0.8, 0.8, 0.8)))))
    assert st["rays"] > st0["rays"]


# ---- materials at the edges against the second reading

def rust_min(a, b):
    """f64::min: a NaN operand is ignored."""
    return b if a != a else (a if b != b else (a if a < b else b))


def rust_max(a, b):
    return b if a != a else (a if b != b else (a if a > b else b))


_NP_MATH = types.SimpleNamespace(sqrt=np.sqrt, tan=np.tan, acos=np.arccos, exp=np.exp, log=np.log, cos=np.cos,
                                 sin=np.sin, pi=np.pi, isinf=np.isinf, floor=np.floor, ceil=np.ceil, atan2=np.arctan2)


@contextlib.contextmanager
def ieee_second_reading():
    """The second reading of material.rs evaluated in IEEE arithmetic: math.* replaced by numpy's ufuncs (inf and NaN
    where math.* raises), min with f64::min's NaN rule, inputs as np.float64 (x / 0.0 is inf, not an exception)."""
    saved = M2.math, getattr(M2, "min", None)
    M2.math, M2.min = _NP_MATH, rust_min
    try:
        with np.errstate(all="ignore"):
            yield
    finally:
        M2.math = saved[0]
        if saved[1] is None:
            del M2.min
        else:
            M2.min = saved[1]


def f64_material(m):
    f = np.float64
    return types.SimpleNamespace(kind=m.kind, metallic=m.metallic, color=tuple(f(c) for c in m.color),
                                 spec_color=tuple(f(c) for c in m.spec_color), alpha=f(m.alpha), ior=f(m.ior),
                                 r0=tuple(f(c) for c in m.r0))


# ior exactly 1: the refracted light is -view up to rounding, and the btdf's half vector -view - light
# (material.rs:1386-1390) is the rounding residue, which the two readings' last bits decide.  Those two are compared
# with the oracle on the GPU only (bit for bit), not with the second reading
ILL_CONDITIONED = {"ctg_ior_1", "ctr_ior_1"}


@pytest.mark.parametrize("name", [m for m in N.EDGE_MATERIALS if m not in ILL_CONDITIONED])
def test_edge_material_lands_on_the_second_reading(name):
    mat = N.EDGE_MATERIALS[name]
    nrm, view, key = N.edge_normals_views(1500, seed=23)
    sc, col, dr, nd = _oracle.material_evaluate(mat, nrm, view, key)
    m = f64_material(mat)
    checked = nan_seen = 0
    with ieee_second_reading():
        for i in range(len(key)):
            try:
                out, draws = M2.evaluate(m, tuple(nrm[i]), tuple(view[i]), key[i])
            except M2.Skip:
                continue  # a decision within 1e-9 of its threshold
            checked += 1
            assert (out is not None) == bool(sc[i]), (name, i)
            assert draws == nd[i], (name, i)
            if out is None:
                continue
            color, light = np.array(out[0], dtype=np.float64), np.array(out[1], dtype=np.float64)
            assert np.array_equal(np.isnan(color), np.isnan(col[i])), (name, i, color, col[i])
            ok = ~np.isnan(color)
            nan_seen += int((~ok).any())
            assert np.allclose(col[i][ok], color[ok], rtol=1e-9, atol=1e-300), (name, i, col[i], color)
            assert np.array_equal(np.isnan(light), np.isnan(dr[i])), (name, i, light, dr[i])
            lk = ~np.isnan(light)
            assert np.allclose(dr[i][lk], light[lk], rtol=0, atol=1e-9), (name, i, dr[i], light)
    assert checked > 0.9 * len(key), checked
    if "alpha_1e-200" in name or "alpha_1e-160" in name:
        assert nan_seen > 0, "the edge produced no NaN colour"


# ---- background of odd HDRIs against the second reading

@contextlib.contextmanager
def rust_clip_second_reading():
    """lib_rs's texel clip read with f64::min / f64::max (NaN ignored) in the Rust order, clip(0, 3) =
    x.min(3).max(0) (vecmath.rs:388-396): NaN -> 3, +inf and FLT_MAX -> 3, -inf and negatives -> 0."""
    saved = L2.background

    def background(hdri, d):
        return saved(np.vectorize(lambda c: rust_max(rust_min(float(c), 3.0), 0.0))(hdri.astype(np.float64)), d)
    L2.background = background
    try:
        yield background
    finally:
        L2.background = saved


def test_rust_clip_of_special_texels():
    got = [rust_max(rust_min(float(c), 3.0), 0.0) for c in (np.nan, np.inf, -np.inf, -1.5, 7.25, 3.0, N.F32_MAX,
                                                           N.F32_SUB, 0.5)]
    assert got == [3.0, 3.0, 0.0, 0.0, 3.0, 3.0, 3.0, N.F32_SUB, 0.5]


@pytest.mark.parametrize("shape", list(N.odd_hdris()))
def test_background_of_odd_hdris_lands_on_the_second_reading(shape):
    hdri = N.odd_hdris()[shape]
    assert np.isnan(hdri).any() and np.isinf(hdri).any() and (hdri < 0).any() and (hdri > 3).any()
    h, w = hdri.shape[:2]
    from rayrs_amd.api import BvhHeuristic, Emission, Material, Object
    osc = _oracle.OracleScene([Object.sphere(1.0, (0.0, 1.0, 0.0), Material.NoReflect(), Emission.Dark())], 1e-6, 1e6,
                              BvhHeuristic.Midpoint, hdri)
    d = N.background_dirs_for(w, h, n=600)
    got = osc.background(d)
    assert np.isfinite(got).all() and (got >= 0).all() and (got <= 3.0).all()
    with rust_clip_second_reading() as bg:
        for k in range(len(d)):
            assert np.allclose(got[k], bg(hdri, tuple(d[k])), rtol=1e-9, atol=1e-300), (shape, k, d[k])


# ---- f32-subnormal coordinates

def test_f32_subnormal_coordinates_keep_the_compact_layout():
    cam_args, objs, heur, hdri = N.subnormal_coordinate_scene()
    assert any(o.kind == "triangle" and N.F32_SUB in [c for p in o.p for c in p] for o in objs)
    scene = rayrs_amd.Scene(objs, 1e-6, 1e6, heur, hdri, device=-1)
    assert scene.info()["compact"] == 1
    _, _, ref, st = oracle_frame((cam_args, objs, heur, hdri))
    assert np.isfinite(ref).all() and st["escaped_paths"] < st["paths"]
