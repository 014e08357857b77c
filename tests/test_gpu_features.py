"""First-hit feature buffers on the GPU (include/rayrs_hip.h FEATURES), held to the CPU oracle bit for bit: all five planes,
on the local-pool scene and the streaming one with a hot group, for 1, 5 and 16 samples, both walks, a ragged image, tile
shares, every material kind; a film's features are render_features with the film's settings; and nothing a film or a
render returns depends on whether features or a denoise were asked for in between."""
import numpy as np
import pytest

import _features as F
import _film
import rayrs_amd
from rayrs_amd import procedural, scenes
from rayrs_amd.api import Fresnel, Material

pytestmark = pytest.mark.gpu

SEED, BOUNCES, C = _film.SEED, _film.BOUNCES, _film.C
COUNTS = (1, 5, 16)


def gpu_of(desc):
    cam_args, objs, heur, env = desc
    return rayrs_amd.Scene(objs, 1e-6, 1e6, heur, env, device=0), rayrs_amd.Camera(*cam_args)


def assert_same_planes(got, want, what):
    assert sorted(got) == sorted(F.PLANES)
    for k in F.PLANES:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        if not F.same_bits(got[k], want[k]):
            bad = got[k] != want[k]
            bad = bad.any(axis=2) if bad.ndim == 3 else bad
            raise AssertionError(f"{what}: plane {k}: {int(bad.sum())} of {bad.size} pixels differ; first at "
                                 f"{np.argwhere(bad)[0] if bad.any() else 'a NaN or a zero sign'}")


@pytest.mark.parametrize("name", ["sphere", "mesh"])
def test_features_equal_the_oracles(name):
    scene, cam = gpu_of(_film.DESCS[name]())
    info = scene.info()
    assert info["local_pool"] == (1 if name == "sphere" else 0)
    if name == "mesh":
        assert info["hot_count"] > 0
    ps = F.named_samples(name, max(COUNTS))
    for n in COUNTS:
        want = F.features_from(ps, n)
        assert_same_planes(rayrs_amd.render_features(scene, cam, samples=n, seed=SEED), want, (name, n))
        assert_same_planes(rayrs_amd.render_features(scene, cam, samples=n, seed=SEED, fast_traversal=True), want,
                           (name, n, "fast walk"))
    # the planes are not trivial on these scenes
    f = F.features_from(ps, 16)
    assert 0 < (f["object"] != F.MISS).sum() and len(np.unique(f["object"])) >= 2
    assert len(np.unique(f["depth"])) > 16 and (np.abs(f["normal"]).sum(axis=2) > 0.0).any()
    # another seed gives other samples
    other = rayrs_amd.render_features(scene, cam, samples=5, seed=SEED + 1)
    assert not F.same_bits(other["depth"], F.features_from(ps, 5)["depth"])


@pytest.mark.parametrize("name", ["sphere", "mesh"])
def test_a_ragged_image_and_tile_shares(name):
    w, h = 37, 19   # neither side a multiple of 8
    scene, cam = gpu_of(_film.DESCS[name](w, h))
    assert (cam.x_pixels(), cam.y_pixels()) == (w, h)
    ps = F.named_samples(name, 5, w, h)
    whole = F.features_from(ps, 5)
    assert_same_planes(rayrs_amd.render_features(scene, cam, samples=5, seed=SEED), whole, (name, "ragged"))
    total = {k: np.zeros_like(whole[k]) for k in ("normal", "albedo", "depth", "coverage")}
    seen = np.zeros((h, w), dtype=np.int64)
    for rank in range(3):
        part = rayrs_amd.render_features(scene, cam, samples=5, seed=SEED, tile_rank=rank, tile_ranks=3)
        assert_same_planes(part, F.features_from(ps, 5, rank, 3), (name, "rank", rank))
        mask = rayrs_amd.tiles.tile_mask(w, h, rank, 3)
        for k in total:
            assert (part[k][~mask] == 0.0).all() and not np.signbit(part[k][~mask]).any()   # +0 outside the share
            total[k] += part[k]
        assert (part["object"][~mask] == F.MISS).all()
        seen += mask
    assert (seen == 1).all()
    for k in total:   # the three shares add up to the whole frame (every pixel is non-zero in one of them at most)
        assert np.array_equal(total[k], whole[k]), k


def nine_kinds():
    """A row of spheres, one per material kind, each with a colour of its own."""
    mats = [Material.LambertianDiffuse((0.8, 0.7, 0.6)), Material.Reflect((0.1, 0.2, 0.3)), Material.Refract((0.9, 0.8, 0.7), 1.45),
            Material.Glass((0.4, 0.5, 0.6), 1.45), Material.CookTorrance((0.3, 0.6, 0.9), 0.05, Fresnel.SchlickMetallic((0.8, 0.8, 0.8))),
            Material.CookTorranceRefract((0.2, 0.4, 0.8), 0.05, 1.45), Material.CookTorranceGlass((0.7, 0.1, 0.4), 0.05, 1.45),
            Material.Plastic((0.6, 0.3, 0.1), (1, 1, 1), 0.05, 1.45), Material.NoReflect()]
    assert sorted(m.kind for m in mats) == list(range(9))
    return scenes.multiple_spheres(mats)


@pytest.mark.parametrize("make", [scenes.material_test, nine_kinds], ids=["material_test", "nine_kinds"])
def test_albedo_for_every_material_kind(make):
    cam_args, objs, heur = make()
    desc = (scenes.camera_for_resolution(cam_args, 120, 24), objs, heur, procedural.make_hdri(64, 32))
    scene, cam = gpu_of(desc)
    ps = F.sample_features(desc, 5, seed=11)
    want = F.features_from(ps, 5)
    got = rayrs_amd.render_features(scene, cam, samples=5, seed=11)
    assert_same_planes(got, want, make.__name__)
    flat = rayrs_amd.api.flatten_objects(objs)
    hit = np.unique(got["object"][got["object"] != F.MISS])
    assert {flat[k].mat.kind for k in hit} == {o.mat.kind for o in flat}          # every kind of the scene is seen
    if make is nine_kinds:
        assert {flat[k].mat.kind for k in hit} == set(range(9))
    for k in hit:   # where all five samples hit the object, the albedo is its colour (0 for NoReflect)
        full = (got["object"] == k) & (ps["obj"] == k).all(axis=2)
        if full.any():
            colour = (0.0, 0.0, 0.0) if flat[k].mat.kind == rayrs_amd.api.MAT_NO_REFLECT else flat[k].mat.color
            assert np.abs(got["albedo"][full] - np.array(colour)).max() < 1e-15, k


@pytest.mark.parametrize("name,share", [("sphere", (0, 1)), ("mesh", (0, 1)), ("mesh", (1, 3))])
def test_a_films_features_are_render_features_with_its_settings(name, share):
    scene, cam = gpu_of(_film.DESCS[name]())
    rank, ranks = share
    film = rayrs_amd.Film(scene, cam, sample_chunk=C, max_bounces=BOUNCES, seed=SEED, tile_rank=rank, tile_ranks=ranks)
    ps = F.named_samples(name, 16)

    def check(when):
        for n in (5, 16, 5):   # (a count the film holds, another one, the first again)
            got = film.features(n)
            assert_same_planes(got, rayrs_amd.render_features(scene, cam, samples=n, seed=SEED, tile_rank=rank, tile_ranks=ranks),
                               (name, when, n))
            assert_same_planes(got, F.features_from(ps, n, rank, ranks), (name, when, n, "oracle"))

    check("empty")
    film.render(16)
    check("after a uniform pass")
    active, _ = film.render_adaptive(4, 0.6, 24)   # (takes some of the tiles and not all: tests/_film_adaptive.py's replay)
    assert active > 0
    check("after an adaptive pass")
    film.render(4)
    check("after a pass over differing tiles")


@pytest.mark.parametrize("name", ["sphere", "mesh"])
def test_features_and_denoise_leave_films_and_renders_as_they_are(name):
    scene, cam = gpu_of(_film.DESCS[name]())

    def run(with_extras):
        film = rayrs_amd.Film(scene, cam, sample_chunk=C, max_bounces=BOUNCES, seed=SEED)
        out = []
        if with_extras:
            film.features(5)
        film.render(16)
        if with_extras:
            film.features(16), film.denoised(levels=3), rayrs_amd.render_features(scene, cam, samples=3, seed=1)
        out.append(film.state())
        active, _ = film.render_adaptive(4, 0.6, 24)
        if with_extras:
            film.denoised(levels=2, feature_samples=5, out_f64=True), film.features(1)
        film.render(4)
        out += [active, film.state(), film.image(out_f64=True).tobytes(), film.image().tobytes(), film.status(0.2), film.tile_samples().tobytes()]
        if with_extras:
            rayrs_amd.render_features(scene, cam, samples=2, seed=3, fast_traversal=True)
        img, st = rayrs_amd.render(scene, cam, spp=8, max_bounces=BOUNCES, seed=SEED, sample_chunk=C, out_f64=True)
        out += [img.tobytes(), st["rays"], st["paths"]]
        return out

    plain, extras = run(False), run(True)
    assert len(plain) == len(extras)
    for k, (a, b) in enumerate(zip(plain, extras)):
        assert a == b, (name, k)


def test_film_refusals_on_the_device():
    scene, cam = gpu_of(_film.DESCS["sphere"]())
    L = scene._L
    film = rayrs_amd.Film(scene, cam, sample_chunk=C, max_bounces=BOUNCES, seed=SEED)
    out = np.zeros((cam.y_pixels(), cam.x_pixels(), 3))
    k = (1.0, 1.0, 1.0, 1.0)
    assert L.rayrs_film_denoise(film._h, 16, 5, *k, 1, out.ctypes.data) == -1          # an empty film
    assert L.rayrs_film_features(film._h, 0, None, None, None, None, None) == -1
    assert L.rayrs_film_features(film._h, 1 << 30, None, None, None, None, None) == -1
    film.render(4)
    state = film.state()
    assert L.rayrs_film_denoise(film._h, 16, 0, *k, 1, out.ctypes.data) == -1
    assert L.rayrs_film_denoise(film._h, 16, 17, *k, 1, out.ctypes.data) == -1
    assert L.rayrs_film_denoise(film._h, 0, 5, *k, 1, out.ctypes.data) == -1
    assert L.rayrs_film_denoise(film._h, 16, 5, -1.0, 1.0, 1.0, 1.0, 1, out.ctypes.data) == -1
    assert L.rayrs_film_denoise(film._h, 16, 5, 1.0, 1.0, float("nan"), 1.0, 1, out.ctypes.data) == -1
    assert L.rayrs_film_denoise(film._h, 16, 5, *k, 2, out.ctypes.data) == -1
    assert L.rayrs_film_denoise(film._h, 16, 5, *k, 1, None) == -1
    assert L.rayrs_film_denoise(film._h, 16, 5, *k, 1, out.ctypes.data) == 0
    assert film.state() == state
    shared = rayrs_amd.Film(scene, cam, sample_chunk=C, max_bounces=BOUNCES, seed=SEED, tile_rank=0, tile_ranks=2)
    shared.render(4)
    assert L.rayrs_film_denoise(shared._h, 16, 5, *k, 1, out.ctypes.data) == -1        # the filter needs its neighbours
    assert shared.features(5)["depth"].shape == (cam.y_pixels(), cam.x_pixels())       # ... its features do not
