"""GPU parity in the non-finite corners of the radiance half of the path: surfaces whose parameters pass the
reference's asserts yet make NaN, infinite, huge or f32-subnormal radiance (tests/_nonfinite.py; the CPU side,
test_nonfinite_oracle.py, checks that each family really shows its edge on the oracle).

The GPU is compared with the oracle by the NaN-aware rule (_nonfinite.assert_same_frame_nan_aware: NaN places, every
other component bit for bit).  The GPU compared with itself in the same kernel -- a repeated render, tile shares,
logical ranks -- stays bit for bit, NaN bits included."""
import ctypes as C

import numpy as np
import pytest

import _nonfinite as N
import _oracle
import rayrs_amd
from rayrs_amd import _ffi, io, scenes, tiles
from rayrs_amd.api import Axis, Emission, Fresnel, Material, Object

pytestmark = pytest.mark.gpu

STAT_KEYS = ("rays", "paths", "escaped_paths", "nan_pixels", "neg_pixels")


def on_both(desc):
    cam_args, objs, heur, hdri = desc
    scene = rayrs_amd.Scene(objs, 1e-6, 1e6, heur, hdri, device=0)
    osc = _oracle.OracleScene(objs, 1e-6, 1e6, heur, hdri)
    return scene, rayrs_amd.Camera(*cam_args), osc, _oracle.OracleCamera(*cam_args)


def assert_frame(scene, cam, ref, ost, spp, chunk, what, budget=N.BUDGET):
    img, st = rayrs_amd.render(scene, cam, spp, budget, sample_chunk=chunk, out_f64=True)
    for k in STAT_KEYS:
        assert st[k] == ost[k], (what, k, st[k], ost[k])
    N.assert_same_frame_nan_aware(img, ref, what)
    img32, _ = rayrs_amd.render(scene, cam, spp, budget, sample_chunk=chunk, out_f64=False)
    with np.errstate(over="ignore"):
        N.assert_same_frame_nan_aware(img32, ref.astype(np.float32), what + " f32")
    return img, img32, st


@pytest.mark.parametrize("name", list(N.FAMILIES))
def test_family_frames_match_the_oracle(name):
    """Each family on the local-pool route and the streaming one (set_tuning(local_pool=1)), compact and full
    layouts, sample_chunk 0 and 4, and on the streaming route eager_light 0 and 1."""
    fn, _ = N.FAMILIES[name]
    for full in (False, True):
        desc = N.full_layout(fn()) if full else fn()
        scene, cam, osc, ocam = on_both(desc)
        assert scene.info()["compact"] == (0 if full else 1)
        for chunk in (0, 4):
            ref, ost = osc.render(ocam, N.SPP, N.BUDGET, sample_chunk=chunk)
            scene.set_tuning(local_pool=0)
            scene.lab_set(eager_light=0)
            lp, _, st = assert_frame(scene, cam, ref, ost, N.SPP, chunk, f"{name} full={full} chunk={chunk} local pool")
            assert st["local_pool"] == 1
            again, _ = rayrs_amd.render(scene, cam, N.SPP, N.BUDGET, sample_chunk=chunk, out_f64=True)
            assert np.array_equal(again.view(np.uint64), lp.view(np.uint64))
            scene.set_tuning(local_pool=1)
            frames = []
            for eager in (0, 1):
                scene.lab_set(eager_light=eager)
                img, _, st = assert_frame(scene, cam, ref, ost, N.SPP, chunk,
                                          f"{name} full={full} chunk={chunk} streaming eager={eager}")
                assert st["local_pool"] == 0
                frames.append(img)
            N.assert_same_frame_nan_aware(frames[0], frames[1], "eager against on-demand light")
            N.assert_same_frame_nan_aware(lp, frames[0], "local pool against streaming")


def test_local_pool_segments_are_bit_identical():
    """The local pool split into segments of 65536 items renders the same bits, NaN bits included."""
    scene, cam, osc, ocam = on_both(N.FAMILIES["emit_inf_red"][0]())
    spp = 16   # 96 x 64 x 16 = 98304 items: two segments of 65536
    cam_args = scenes.camera_for_resolution(N.FAMILIES["emit_inf_red"][0]()[0], 96, 64)
    cam, ocam = rayrs_amd.Camera(*cam_args), _oracle.OracleCamera(*cam_args)
    ref, ost = osc.render(ocam, spp, N.BUDGET)
    a, _, st = assert_frame(scene, cam, ref, ost, spp, 0, "one segment")
    assert st["local_pool"] == 1 and st["nan_pixels"] > 0
    scene.lab_set(local_segment_items=65536)
    b, _ = rayrs_amd.render(scene, cam, spp, N.BUDGET, out_f64=True)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_mesh_scene_with_an_edge_floor_reaches_the_hot_group():
    def desc():
        cam_args, objs, heur = scenes.mesh_scene(3, area_light=True)
        objs = list(objs)
        objs[0] = Object.plane(Axis.Y, -25.0, 25.0, -25.0, 25.0, 0.0,
                               Material.CookTorrance(N.ONE, 1e-200, Fresnel.SchlickMetallic((0.8, 0.8, 0.8))),
                               Emission.Dark())
        return scenes.camera_for_resolution(cam_args, 48, 32), objs, heur, N.procedural.make_hdri(64, 32)
    scene, cam, osc, ocam = on_both(desc())
    assert scene.info()["hot_count"] > 0
    for chunk in (0, 4):
        ref, ost = osc.render(ocam, 4, N.BUDGET, sample_chunk=chunk)
        assert ost["nan_pixels"] > 0
        for local_pool in (1, 0):
            scene.set_tuning(local_pool=local_pool)
            _, _, st = assert_frame(scene, cam, ref, ost, 4, chunk, f"mesh chunk={chunk} local_pool={local_pool}")
            if local_pool == 1:
                assert st["hot_group"] == 1


def test_f32_subnormal_coordinates_render_the_oracles_frame():
    scene, cam, osc, ocam = on_both(N.subnormal_coordinate_scene())
    assert scene.info()["compact"] == 1
    for local_pool in (0, 1):
        scene.set_tuning(local_pool=local_pool)
        ref, ost = osc.render(ocam, N.SPP, N.BUDGET)
        assert_frame(scene, cam, ref, ost, N.SPP, 0, f"subnormal coordinates local_pool={local_pool}")


@pytest.mark.parametrize("name", ["ct_alpha_1e-200", "ctg_alpha_1e-200", "emit_inf_red"])
def test_nan_paths_traced_bounce_by_bounce(name):
    """rayrs_test_path_trace, both walks, on samples of NaN pixels: object, t and draw exact, throughput and the
    returned colour NaN-aware."""
    scene, cam, osc, ocam = on_both(N.FAMILIES[name][0]())
    ref, _ = osc.render(ocam, N.SPP, N.BUDGET)
    px = np.argwhere(np.isnan(ref).any(axis=2))[:16]
    assert len(px) > 0
    pix = np.array([(r, c) for r, c in px for _ in range(N.SPP)], dtype=np.uint32)
    sam = np.array([s for _ in px for s in range(N.SPP)], dtype=np.uint32)
    cap = N.BUDGET
    tr = osc.path_traces(ocam, [tuple(p) for p in pix], sam, 0x5EED, N.BUDGET, cap=cap)
    assert np.isnan(tr["thr"]).any() or np.isnan(tr["rgb"]).any()   # (an emission of inf * 0 makes the light NaN)
    packed = np.ascontiguousarray((pix[:, 0] << 16) | pix[:, 1], dtype=np.uint32)
    ks = np.ascontiguousarray(sam)
    k = len(pix)
    for exact in (0, 1):
        n = np.zeros(k, dtype=np.uint32); obj = np.zeros((k, cap), dtype=np.int64); t = np.zeros((k, cap))
        thr = np.zeros((k, cap, 3)); draw = np.zeros((k, cap), dtype=np.uint32); rgb = np.zeros((k, 3))
        _ffi.check(scene._L.rayrs_test_path_trace(scene._h, C.byref(cam.desc), 0x5EED, N.BUDGET, packed.ctypes.data,
                                                  ks.ctypes.data, k, exact, cap, n.ctypes.data, obj.ctypes.data,
                                                  t.ctypes.data, thr.ctypes.data, draw.ctypes.data, rgb.ctypes.data),
                   "rayrs_test_path_trace")
        assert np.array_equal(n, tr["n"]) and np.array_equal(obj, tr["obj"]) and np.array_equal(draw, tr["draw"])
        assert np.array_equal(t.view(np.uint64), np.ascontiguousarray(tr["t"]).view(np.uint64))
        N.assert_same_frame_nan_aware(thr, np.ascontiguousarray(tr["thr"]), f"throughput exact={exact}")
        N.assert_same_frame_nan_aware(rgb, np.ascontiguousarray(tr["rgb"]), f"colour exact={exact}")


@pytest.mark.parametrize("name", list(N.EDGE_MATERIALS))
def test_edge_material_against_the_oracle(name):
    mat = N.EDGE_MATERIALS[name]
    normal, view, key = N.edge_normals_views()
    n = len(key)
    sc = np.zeros(n, dtype=np.int32); col = np.zeros((n, 3)); dr = np.zeros((n, 3)); nd = np.zeros(n, dtype=np.uint32)
    m = mat.desc()
    _ffi.check(_ffi.lib().rayrs_test_material(0, C.byref(m), normal.ctypes.data, view.ctypes.data, key.ctypes.data,
                                              n, sc.ctypes.data, col.ctypes.data, dr.ctypes.data, nd.ctypes.data),
               "rayrs_test_material")
    rsc, rcol, rdr, rnd = _oracle.material_evaluate(mat, normal, view, key)
    assert np.array_equal(sc, rsc) and np.array_equal(nd, rnd)
    hit = rsc == 1
    N.assert_same_frame_nan_aware(np.ascontiguousarray(col[hit]), np.ascontiguousarray(rcol[hit]), name + " colour")
    N.assert_same_frame_nan_aware(np.ascontiguousarray(dr[hit]), np.ascontiguousarray(rdr[hit]), name + " direction")


@pytest.mark.parametrize("shape", list(N.odd_hdris()))
def test_background_of_odd_hdris_bit_exact(shape):
    hdri = N.odd_hdris()[shape]
    h, w = hdri.shape[:2]
    objs = [Object.sphere(1.0, (0.0, 1.0, 0.0), Material.NoReflect(), Emission.Dark())]
    scene = rayrs_amd.Scene(objs, 1e-6, 1e6, rayrs_amd.BvhHeuristic.Midpoint, hdri, device=0)
    osc = _oracle.OracleScene(objs, 1e-6, 1e6, rayrs_amd.BvhHeuristic.Midpoint, hdri)
    d = N.background_dirs_for(w, h)
    out = np.zeros_like(d)
    _ffi.check(scene._L.rayrs_test_background(scene._h, d.ctypes.data, len(d), out.ctypes.data),
               "rayrs_test_background")
    want = osc.background(d)
    assert np.isfinite(want).all()
    assert np.array_equal(out.view(np.uint64), want.view(np.uint64))


def test_shares_of_a_nan_and_inf_frame_are_bit_identical():
    """Tile shares (three ranks) placed by their tile masks, and rayrs_render_multi on two and three logical ranks,
    give the single-device frame bit for bit, NaN bits included."""
    scene, cam, osc, ocam = on_both(N.FAMILIES["emit_inf_red"][0]())
    full, st = rayrs_amd.render(scene, cam, N.SPP, N.BUDGET, sample_chunk=4, out_f64=False)
    full64, _ = rayrs_amd.render(scene, cam, N.SPP, N.BUDGET, sample_chunk=4, out_f64=True)
    assert np.isnan(full).any() and np.isinf(full).any()
    for dt, whole in ((np.float32, full), (np.float64, full64)):
        ui = np.uint32 if dt == np.float32 else np.uint64
        got = np.zeros_like(whole)
        for r in range(3):
            p, _ = rayrs_amd.render(scene, cam, N.SPP, N.BUDGET, sample_chunk=4, tile_rank=r, tile_ranks=3,
                                    out_f64=dt == np.float64)
            mask = tiles.tile_mask(N.W, N.H, r, 3)
            got[mask] = p[mask]
        assert np.array_equal(got.view(ui), whole.view(ui))
    clones = [scene] + [scene.clone_to_device(0) for _ in range(2)]
    for k in (2, 3):
        img, mst = rayrs_amd.render_multi(clones[:k], cam, N.SPP, N.BUDGET, sample_chunk=4)
        assert np.array_equal(img.view(np.uint32), full.view(np.uint32)), k
        assert mst["nan_pixels"] == st["nan_pixels"] and mst["rays"] == st["rays"]
        img64, _ = rayrs_amd.render_multi(clones[:k], cam, N.SPP, N.BUDGET, sample_chunk=4, out_f64=True)
        assert np.array_equal(img64.view(np.uint64), full64.view(np.uint64)), k


@pytest.mark.parametrize("name", ["emit_inf_red", "emit_1e308", "plastic_alpha_1e-200", "emit_1e-40"])
def test_writers_on_the_gpu_frame_equal_the_oracles(name, tmp_path):
    scene, cam, osc, ocam = on_both(N.FAMILIES[name][0]())
    img32, _ = rayrs_amd.render(scene, cam, N.SPP, N.BUDGET, out_f64=False)
    ref, _ = osc.render(ocam, N.SPP, N.BUDGET)
    with np.errstate(over="ignore"):
        ref32 = ref.astype(np.float32)
    b_gpu, c_gpu = io.to_raw_bytes(img32)
    b_ref, c_ref = io.to_raw_bytes(ref32)
    assert np.array_equal(b_gpu, b_ref) and c_gpu == c_ref
    io.save_png(tmp_path / "g.png", b_gpu)
    io.save_png(tmp_path / "r.png", b_ref)
    assert (tmp_path / "g.png").read_bytes() == (tmp_path / "r.png").read_bytes()
    io.save_hdr(tmp_path / "g.hdr", img32)
    io.save_hdr(tmp_path / "r.hdr", ref32)
    assert (tmp_path / "g.hdr").read_bytes() == (tmp_path / "r.hdr").read_bytes()
