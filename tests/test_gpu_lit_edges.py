"""The lit radiance kernels (radiance_lit.hip, include/rayrs_hip.h LIGHT SAMPLING) on the branches tests/test_gpu_lit.py never
takes, bit for bit and count for count against the plain-Python reading (tests/_lit.py): a rectangle lamp on every axis and a
list of K = RAYRS_MAX_LIGHTS (the lamp box, tests/_lit.py lamp_box), paths that end at the bounce budget, lane stacks spilled to
HBM, the image form on the fast walk and across launches, points and normals as given, and the open z window (0, inf).

The inputs and the reading's answers need no device (inputs(), expected() on the default walk): tests/test_lit_edges.py asserts
from them, without a GPU, that the comparisons below are not vacuous.  The scenes on the device live in this file's own
families, so a lab knob left set here cannot reach tests/test_gpu_lit.py."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import _lit
import _nonfinite_rays as N
import _oracle
import _radiance
import rayrs_amd
from _nonfinite import assert_same_frame_nan_aware
from rayrs_amd import procedural, scenes
from rayrs_amd.api import Material
from test_gpu_radiance import primary_rays

pytestmark = pytest.mark.gpu

HDRI = procedural.make_hdri(128, 64)
WINDOWS = {"std": (1e-6, 1e6), "open": (0.0, float("inf"))}
S = 5
SEED = 0x5EED
W, H = 32, 24
BIAS = 1e-4
AXES = tuple(r[0] for r in _lit.LAMP_BOX_RECTS)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def frozen(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    a.setflags(write=False)
    return a


# ------------------------------------------------------------------------------------------------------ inputs (no device)

def inputs(name, window="std"):
    return _inputs(name, window)   # (one cache entry however the default is spelt)


@functools.lru_cache(maxsize=None)
def _inputs(name, window):
    """A family's objects, rays, points, light lists and its reading on the default walk.  "box": the lamp box, the list "all" of
    K = 8, one list of K = 1 per axis, and "x8", the X rectangle eight times.  "mesh3_light": the streaming route's scene with a
    hot group, its list emitters(objs).  "single": scenes.single_sphere with a Lambertian sphere, which is the list."""
    z_near, z_far = WINDOWS[window]
    if name == "box":
        cam_args, objs, heur, names = _lit.lamp_box()
        lists = {"all": names["lights"], "x8": (names["rect"]["X"],) * 8}
        lists.update({a: (names["rect"][a],) for a in AXES})
        x = np.linspace(-3.5, 3.5, 8)
    elif name == "mesh3_light":
        cam_args, objs, heur = scenes.mesh_scene(3, Material.LambertianDiffuse((0.8, 0.8, 0.8)), area_light=True)
        lists = {"emitters": tuple(rayrs_amd.emitters(objs))}
        x = np.linspace(-4.0, 4.0, 8)
    else:
        cam_args, objs, heur = scenes.single_sphere(Material.LambertianDiffuse((0.8, 0.6, 0.4)))
        lists = {"sphere": (1,)}
        x = np.linspace(-4.0, 4.0, 8)
    o, d = primary_rays(cam_args, W, H)
    p = frozen([(xi, 0.0, zi) for zi in x for xi in x])
    nrm = frozen(np.tile((0.0, 1.0, 0.0), (len(p), 1)))
    host = rayrs_amd.Scene(objs, z_near, z_far, heur, HDRI, device=-1)
    return SimpleNamespace(name=name, objs=objs, heur=heur, z=(z_near, z_far), raw_cam_args=cam_args,
                           cam_args=scenes.camera_for_resolution(cam_args, W, H), o=o, d=d, p=p, nrm=nrm, lists=lists,
                           host_info=host.info(), reading=_lit.Reading(objs, z_near, z_far, heur, HDRI), tally=_lit.new_tally())


def family(name, window="std"):
    return _family(name, window)


@functools.lru_cache(maxsize=None)
def _family(name, window):
    """The family on the device, with the reading of each walk (the fast walk's on the product's records, the recipe of
    tests/test_gpu_render.py)."""
    i = inputs(name, window)
    scene = rayrs_amd.Scene(i.objs, i.z[0], i.z[1], i.heur, HDRI, device=0)
    fast_osc = _oracle.OracleScene(i.objs, i.z[0], i.z[1], i.heur, HDRI).use_product_walk(scene, fast=True)
    readings = {False: i.reading, True: _lit.Reading(i.objs, i.z[0], i.z[1], i.heur, HDRI, osc=fast_osc, traversal=2)}
    return SimpleNamespace(i=i, scene=scene, readings=readings, info=scene.info(), walks={})


@functools.lru_cache(maxsize=None)
def edge_points():
    """The points and normals of test_normals_and_points_as_given, on the lamp box: (points, normals) of 64 oblique unit normals
    (a fixed-seed generator, any direction: half of them look below the floor they stand on) and 64 non-unit normals of lengths
    0.5 and 3 by turns, at the box's floor points twice over."""
    i = inputs("box")
    r = np.random.default_rng(20252)
    n = r.normal(size=(128, 3))
    n /= np.linalg.norm(n, axis=1)[:, None]
    n[64:, 1] = np.abs(n[64:, 1])
    n[64::2] *= 0.5
    n[65::2] *= 3.0
    return frozen(np.concatenate([i.p, i.p])), frozen(n)


@functools.lru_cache(maxsize=None)
def corrupted_points():
    """tests/_nonfinite_rays.py's families applied to (points, normals) in runs of 64: (points, normals, touched)."""
    i = inputs("box")
    p, n, touched = N.corrupt_in_runs(i.p, edge_points()[1][:64], i.host_info["root_box"], 64)
    return frozen(p), frozen(n), touched


def reading_of(name, fast, window):
    return family(name, window).readings[True] if fast else inputs(name, window).reading


def expected(name, which, what, fast=False, max_bounces=50, window="std"):
    return _expected(name, which, what, bool(fast), int(max_bounces), window)


@functools.lru_cache(maxsize=None)
def _expected(name, which, what, fast, max_bounces, window):
    """The reading's paths of the family's rays (what = "radiance"), points ("irradiance") or pixels ("image"): (values,
    queries).  The default walk's 50-bounce paths under the standard window feed the family's tally."""
    i = inputs(name, window)
    R = reading_of(name, fast, window)
    lights = i.lists[which]
    tally = i.tally if not fast and max_bounces == 50 and window == "std" else None
    if what == "radiance":
        return _lit.radiance_paths(R, i.o, i.d, S, max_bounces, SEED, lights, tally=tally)
    if what == "irradiance":
        return _lit.irradiance_paths(R, i.p, i.nrm, S, BIAS, max_bounces, SEED, lights, tally=tally)
    return _lit.image_paths(R, _oracle.OracleCamera(*i.cam_args), S, max_bounces, SEED, lights, tally=tally)


def rays_differing(a, b):
    """How many rays' answers differ in bits between two sets of paths (sample_chunk 0)."""
    ra, rb = _radiance.answers(*a, 0)[0], _radiance.answers(*b, 0)[0]
    return int((bits(ra) != bits(rb)).any(axis=1).sum())


def check(got, values, queries, chunk, what):
    rad, cnt = got
    want_rad, want_cnt = _radiance.answers(values, queries, chunk)
    assert rad.dtype == np.float64 and cnt.dtype == np.uint32 and rad.shape == want_rad.shape and cnt.shape == want_cnt.shape, what
    bad = np.flatnonzero(cnt != want_cnt)
    assert len(bad) == 0, (what, "queries", len(bad), [(int(i), int(cnt[i]), int(want_cnt[i])) for i in bad[:5]])
    assert_same_frame_nan_aware(rad, want_rad, str(what))


def run(f, what, which, chunk, fast=False, max_bounces=50, cam_args=None):
    """One call of the form `what` on the family's own inputs: (radiance (n, 3), queries (n,))."""
    i = f.i
    kw = dict(max_bounces=max_bounces, seed=SEED, sample_chunk=chunk, fast_traversal=fast, queries=True)
    if what == "radiance":
        return f.scene.radiance(i.o, i.d, samples=S, lights=i.lists[which], **kw)
    if what == "irradiance":
        return f.scene.irradiance(i.p, i.nrm, samples=S, bias=BIAS, lights=i.lists[which], **kw)
    cam = rayrs_amd.Camera(*(cam_args or i.cam_args))
    assert (cam.x_pixels(), cam.y_pixels()) == (W, H)
    img, cnt = rayrs_amd.render_lit(f.scene, cam, S, i.lists[which], **kw)
    assert img.shape == (H, W, 3) and cnt.shape == (H, W)
    return img.reshape(-1, 3), cnt.reshape(-1)


def render_walk_is_fast(f, cam_args=None):
    """Whether a render of the family with fast_traversal = 1 takes the fast walk: rayrs_render_stats.exact_walk of such a
    render, as tests/test_gpu_render.py reads it -- never the lit code's own choice."""
    cam_args = cam_args or f.i.cam_args
    if cam_args not in f.walks:
        _, st = rayrs_amd.render(f.scene, rayrs_amd.Camera(*cam_args), 1, seed=SEED, out_f64=True, fast_traversal=True)
        assert st["local_pool"] == f.info["local_pool"]
        f.walks[cam_args] = st["exact_walk"] == 0
    return f.walks[cam_args]


def image_walk(f, fast):
    """The walk (False: default, True: fast) whose reading the image form is held to when `fast` is asked for."""
    return bool(fast) and render_walk_is_fast(f)


FORMS = ("radiance", "irradiance", "image")


def assert_routes():
    box, mesh = family("box"), family("mesh3_light")
    assert box.info["local_pool"] == 1 and box.info["compact"] == 0 and mesh.info["local_pool"] == 0 and mesh.info["hot_count"] >= 1


# ------------------------------------------------------------------------------------------------------ 1: every axis, K = 8

@pytest.mark.parametrize("what", FORMS)
def test_all_axes_and_eight_lights_are_the_readings(what):
    """The lamp box with the list of all eight lamps, on both walks (the image: fast_traversal 0 and 1, held to the walk a render
    takes), sample_chunk 0 and 2."""
    assert_routes()
    f = family("box")
    assert len(f.i.lists["all"]) == 8 == len(set(f.i.lists["all"]))
    for fast in (False, True):
        values, queries = expected("box", "all", what, image_walk(f, fast) if what == "image" else fast)
        for chunk in (0, 2):
            check(run(f, what, "all", chunk, fast), values, queries, chunk, ("box", what, fast, chunk))
    if what == "radiance":
        unlit = f.scene.radiance(f.i.o, f.i.d, samples=S, seed=SEED)
        lit = f.scene.radiance(f.i.o, f.i.d, samples=S, seed=SEED, lights=f.i.lists["all"])
        assert (bits(unlit) != bits(lit)).any(axis=1).sum() >= 100   # (the lights change the answers)


@pytest.mark.parametrize("which", AXES + ("x8",))
def test_one_rectangle_of_each_axis_alone_is_the_readings(which):
    """K = 1, the rectangle of one axis: a failure names its axis.  x8: K = 8, the X rectangle eight times.  The points beside
    the rays: a point's first direction is traced whatever its colour is, where a ray's aimed bounce mostly ends at the roulette
    before it is (a small far lamp's density makes the colour small), so the points are what tells the axes apart
    (tests/test_lit_edges.py counts it)."""
    f = family("box")
    for what in ("radiance", "irradiance"):
        values, queries = expected("box", which, what)
        check(run(f, what, which, 2), values, queries, 2, ("box", which, what))
    if which == "x8":   # (the same picks and directions as K = 1; the density is p summed eight times and divided by 8.0)
        assert len(f.i.lists["x8"]) == 8
        print("x8 against X alone: rays that differ", rays_differing(expected("box", "x8", "radiance"), expected("box", "X", "radiance")))


# ------------------------------------------------------------------------------------------------------ 2: the bounce budget

@pytest.mark.parametrize("name,which", [("box", "all"), ("mesh3_light", "emitters")])
@pytest.mark.parametrize("max_bounces", [1, 2, 3])
def test_paths_that_end_at_the_bounce_budget_are_the_readings(name, which, max_bounces):
    """max_bounces 1, 2 and 3: `result = light` at the budget, and for the points `first * light`.  From the reading: over the
    rays, the points and the pixels together, 50 answers and more are not the 50-bounce answers, one of them a point's."""
    f = family(name)
    differing = {}
    for what in FORMS:
        for fast in (False, True):
            values, queries = expected(name, which, what, image_walk(f, fast) if what == "image" else fast, max_bounces)
            assert queries.max() == max_bounces
            if not fast:
                differing[what] = rays_differing((values, queries), expected(name, which, what, False, 50))
                print(name, what, "max_bounces", max_bounces, "paths at the budget", int((queries == max_bounces).sum()),
                      "answers that differ from 50 bounces", differing[what])
            check(run(f, what, which, 2, fast, max_bounces), values, queries, 2, (name, what, fast, max_bounces))
    assert sum(differing.values()) >= 50 and differing["irradiance"] >= 1
    values, queries = expected(name, which, "irradiance", False, max_bounces)
    check(run(f, "irradiance", which, 0, False, max_bounces), values, queries, 0, (name, "irradiance", "chunk 0", max_bounces))


# ------------------------------------------------------------------------------------------------------ 3: stacks in HBM

@pytest.mark.parametrize("knobs", [(0, 0, 0), (1, 64, 1), (64, 1, 64)], ids=["default", "1-64-1", "64-1-64"])
def test_stacks_spilled_to_hbm_give_the_same_bits(knobs):
    """stack_lds = 2 on mesh3_light: all but two entries of a lane's stack live in the strip the scene keeps for the queries
    (tests/test_gpu_radiance.py test_every_threshold_gives_the_same_bits does this to the unlit kernel on mesh4)."""
    f = family("mesh3_light")
    assert f.info["wide_depth"] > 2 and (f.info["hot_depth"] if f.info["hot_count"] else f.info["gate_depth"]) > 2
    try:
        f.scene.lab_set(stack_lds=2)
        f.scene.lab_radiance_tuning(*knobs)
        for what in FORMS:
            for fast in (False, True):
                values, queries = expected("mesh3_light", "emitters", what, image_walk(f, fast) if what == "image" else fast)
                check(run(f, what, "emitters", 2, fast), values, queries, 2, ("stack_lds=2", knobs, what, fast))
    finally:
        f.scene.lab_radiance_tuning(0, 0, 0)
        f.scene.lab_set()


# ------------------------------------------------------------------------------------------------------ 4: the image's walk

def far_camera(f):
    """tests/test_gpu_render.py's long lens from 12 root-box diagonals above the floor's corner, at this file's image size."""
    box = np.array(f.info["root_box"])
    diag = float(np.linalg.norm(box[1::2] - box[0::2]))
    origin = (float(box[1] + 12.0 * diag * 0.6), float(12.0 * diag * 0.8), 0.3)
    return (origin, (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), 0.45, W / 254.0, H / 254.0, 100)


def test_the_lit_image_on_the_fast_walk_is_the_reading_of_the_walk_a_render_takes():
    """include/rayrs_hip.h IMAGE FORM: "fast_traversal is treated as rayrs_render_ao treats it: the walk is the one a render with
    these settings takes (the camera rule of rayrs_render_params.fast_traversal included), for the whole path".  Which walk that
    is comes from rayrs_render_stats.exact_walk of a render with these settings.  mesh3_light from the reference's camera: the
    fast walk; from 12 diagonals away: the default walk whatever was asked.  The lamp box rests on rayrs_render_stats.exact_walk's
    "the local-pool route never makes the bets": its frame with fast_traversal = 1 is the frame without it.  Both walks find the
    same closest hits (that is their contract), so the readings of the two agree where neither bet fails and the count printed
    below may be 0: what this test adds is the lit evaluation on the fast walk's kernels from the pixel start, never run before."""
    assert_routes()
    mesh, box = family("mesh3_light"), family("box")
    assert render_walk_is_fast(mesh)
    values, queries = expected("mesh3_light", "emitters", "image", True)
    for chunk in (0, 2):
        check(run(mesh, "image", "emitters", chunk, True), values, queries, chunk, ("mesh3_light", "fast image", chunk))
    print("mesh3_light: pixels whose fast-walk reading differs from the default walk's",
          rays_differing((values, queries), expected("mesh3_light", "emitters", "image", False)))
    # the camera rule
    far = far_camera(mesh)
    assert not render_walk_is_fast(mesh, far)
    lights = mesh.i.lists["emitters"]
    values, queries = _lit.image_paths(mesh.readings[False], _oracle.OracleCamera(*far), S, 50, SEED, lights)
    assert (queries >= 2).sum() >= 100   # (the lens does see the scene)
    check(run(mesh, "image", "emitters", 2, True, cam_args=far), values, queries, 2, ("mesh3_light", "far camera"))
    # the local-pool route
    assert not render_walk_is_fast(box)
    values, queries = expected("box", "all", "image", False)
    plain, asked = run(box, "image", "all", 2, False), run(box, "image", "all", 2, True)
    assert plain[0].tobytes() == asked[0].tobytes() and np.array_equal(plain[1], asked[1])
    check(asked, values, queries, 2, ("box", "fast image"))


# ------------------------------------------------------------------------------------------------------ 5: an image of two launches

def test_an_image_of_more_than_a_launch():
    """S = 1: an item a pixel and 2^20 of them a launch; 1025 x 1024 pixels are 1024 more.  The second launch's pixels are
    index_base + ray."""
    i = inputs("single")
    scene = rayrs_amd.Scene(i.objs, i.z[0], i.z[1], i.heur, HDRI, device=0)
    cam_args = scenes.camera_for_resolution(i.raw_cam_args, 1025, 1024)
    cam, ocam = rayrs_amd.Camera(*cam_args), _oracle.OracleCamera(*cam_args)
    npix = 1025 * 1024
    assert (cam.x_pixels(), cam.y_pixels()) == (ocam.x_pixels(), ocam.y_pixels()) == (1025, 1024) and 1 << 20 < npix < (1 << 20) + 2000
    lights = i.lists["sphere"]
    img, cnt = rayrs_amd.render_lit(scene, cam, 1, lights, seed=SEED, queries=True)
    img, cnt = img.reshape(-1, 3), cnt.reshape(-1)
    deep = 0
    for a in (0, (1 << 20) - 32, npix - 64):
        pixels = range(a, a + 64)
        values, queries = _lit.image_paths(i.reading, ocam, 1, 50, SEED, lights, pixels=pixels)
        check((img[a:a + 64], cnt[a:a + 64]), values, queries, 0, ("pixels from", a))
        deep += int((queries >= 2).sum())
    # a run of the sphere's own pixels, in the first launch, so that the three runs above are not all sky and floor
    a = 512 * 1025 + 480
    values, queries = _lit.image_paths(i.reading, ocam, 1, 50, SEED, lights, pixels=range(a, a + 64))
    check((img[a:a + 64], cnt[a:a + 64]), values, queries, 0, ("pixels from", a))
    print("paths of two queries and more in the three runs", deep, "and in the middle run", int((queries >= 2).sum()))
    assert deep >= 32
    plain, st = rayrs_amd.render(scene, cam, 1, seed=SEED, out_f64=True)
    lit, cnt0 = rayrs_amd.render_lit(scene, cam, 1, [], seed=SEED, queries=True)
    assert plain.tobytes() == lit.tobytes() and int(cnt0.sum(dtype=np.uint64)) == st["rays"]
    assert (bits(img) != bits(lit.reshape(-1, 3))).any(axis=1).sum() >= 1000   # (the list changes the frame)


# ------------------------------------------------------------------------------------------------------ 6: points and normals as given

def test_normals_and_points_as_given():
    """Lit irradiance on the lamp box, default walk: oblique unit normals, non-unit normals, floor points with bias 0, and the
    non-finite and far-scaled families of tests/_nonfinite_rays.py on (points, normals).  NaN places must coincide."""
    f = family("box")
    R, lights = f.readings[False], f.i.lists["all"]
    p, n = edge_points()
    cp, cn, touched = corrupted_points()
    cases = [("oblique and non-unit", p, n, BIAS), ("bias 0", f.i.p, f.i.nrm, 0.0), ("bias 0, oblique", p[:64], n[:64], 0.0),
             ("non-finite", cp, cn, BIAS)]
    for what, pts, nrm, bias in cases:
        samples = 3 if what == "non-finite" else S   # (4,807 inputs: three samples are two chunks of 2 still)
        values, queries = _lit.irradiance_paths(R, pts, nrm, samples, bias, 50, SEED, lights)
        want, _ = _radiance.answers(values, queries, 0)
        print(what, "inputs", len(pts), "NaN answers", int(np.isnan(want).any(axis=1).sum()), "non-zero answers",
              int((want != 0.0).any(axis=1).sum()))
        if what == "non-finite":
            print("touched inputs", int(touched.sum()))
            assert touched.sum() >= 100
        else:
            assert (np.nan_to_num(want) != 0.0).any(axis=1).sum() >= len(pts) // 2
        for chunk in (0, 2):
            check(f.scene.irradiance(pts, nrm, samples=samples, bias=bias, seed=SEED, sample_chunk=chunk, queries=True, lights=lights),
                  values, queries, chunk, (what, chunk))


# ------------------------------------------------------------------------------------------------------ 7: the open window

@pytest.mark.parametrize("name,which", [("box", "all"), ("mesh3_light", "emitters")])
def test_the_open_z_window_is_the_readings(name, which):
    """(z_near, z_far) = (0, inf), as the unlit routes are held to it (tests/test_gpu_nonfinite_rays.py)."""
    f = family(name, "open")
    assert f.i.z == (0.0, float("inf"))
    for what in ("radiance", "irradiance"):
        values, queries = expected(name, which, what, window="open")
        print(name, what, "rays that differ from the window (1e-6, 1e6)", rays_differing((values, queries), expected(name, which, what)))
        for chunk in (0, 2):
            check(run(f, what, which, chunk), values, queries, chunk, (name, "open", what, chunk))
