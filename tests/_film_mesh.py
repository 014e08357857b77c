"""What the mesh-lit films' and bakes' tests (test_gpu_film_mesh.py, test_gpu_bake_mesh.py) expect, from the plain-Python reading
of MESH LIGHTS alone (tests/_mesh.py): the per-sample values and closest-hit query counts of every pixel of a 20 x 12 frame -- 3 x 2
tiles, four padded columns and four padded rows: interior, right-edge, bottom-edge and corner tiles, and items the start skips --
and of 130 rays and 130 points per family, made once per (family, sky, walk) and folded by _film.expectation, _film.noise_counts,
_film_adaptive.Replay and tests/_bake.py's Replay.  Nothing here calls the library under test.

The families are tests/test_gpu_mesh_lights.py's: `room` (f64 records, two lamps plus its group, a listed triangle behind a listed
one), `small` (local-pool-sized: the default walk whatever is asked) and `mesh1` (compact records; streams; a hot group and a fast
walk of its own; every third mesh triangle listed, with its rectangle lamp), all under that file's studio map.  The default walk's
reading is made here from the family's description; the fast walk's needs the device scene, and the GPU tests register it."""
import functools

import numpy as np

import _mesh
import _oracle
import rayrs_amd
from rayrs_amd import scenes

W, H, C = 20, 12, 2
N_MAX = 9          # the longest film and bake of the tests: passes 2 + 4 + 3
SEED, BOUNCES, BIAS = 0x5EED, 50, 1e-4
N_POINTS = 130
SIZES = (1, 63, 64, 65, 130)   # the wave edges
FAMILIES = ("room", "small", "mesh1")
LIST_OF = {"room": "two", "small": "two", "mesh1": "lamp"}


@functools.lru_cache(maxsize=None)
def description(name):
    """(camera args at W x H, objects, heuristic, the group's triangles, the list's lamps) of a family, as
    test_gpu_mesh_lights.family makes its scene."""
    import test_gpu_mesh_lights as T
    if name in ("room", "small"):
        cam_args, objs, heur, names = _mesh.mesh_room(small=name == "small")
        tris, lamps = names["group"], (names["sphere_lamp"], names["rect_lamp"])
    else:
        cam_args, objs, heur, tris = T.mesh1_objects()
        lamps = tuple(rayrs_amd.emitters(objs))
    return scenes.camera_for_resolution(cam_args, W, H), objs, heur, tuple(tris), tuple(lamps)


_fast = {}


def register_fast_walk(name, reading):
    """The family's reading on the product's fast tree (it needs the device scene: the GPU tests bring it)."""
    _fast[name] = reading


@functools.lru_cache(maxsize=None)
def reading(name, fast=False):
    if fast:
        return _fast[name]
    import test_gpu_mesh_lights as T
    cam_args, objs, heur, tris, lamps = description(name)
    return _mesh.Reading(objs, T.Z_NEAR, T.Z_FAR, heur, T.HDRI, list(tris))


def lights(name, sky):
    """The list a Film, a Bake, render_lit or a query takes beside mesh=."""
    return list(description(name)[4]) + ([rayrs_amd.SKY] if sky else [])


def _frozen(values, queries):
    values, queries = np.array(values, dtype=np.float64), np.array(queries).astype(np.uint64)
    assert np.isfinite(values).all()   # every comparison with these is of bits
    values.setflags(write=False), queries.setflags(write=False)
    return values, queries


@functools.lru_cache(maxsize=None)
def image_paths(name, sky, fast=False):
    """(rgb (H, W, N_MAX, 3) f64, queries (H, W, N_MAX) uint64) of the family's frame: sample s of pixel (row, col) as
    rayrs_render_mesh runs it."""
    cam_args = description(name)[0]
    values, queries = _mesh.image_paths(reading(name, fast), _oracle.OracleCamera(*cam_args), N_MAX, BOUNCES, SEED, lights(name, sky))
    return _frozen(np.asarray(values).reshape(H, W, N_MAX, 3), np.asarray(queries).reshape(H, W, N_MAX))


@functools.lru_cache(maxsize=None)
def geometry(name):
    """(origins, directions, points, normals), (130, 3) f64 each, as tests/_bake.py makes them: 130 rays of a fan of 40 x 24 from
    the family's camera that hit something, spread evenly over them, and their closest hits with the normal back along the ray."""
    import test_gpu_mesh_lights as T
    cam_args, objs, heur, tris, lamps = description(name)
    eye, up, lookat = (np.asarray(cam_args[k], dtype=np.float64) for k in (0, 1, 2))
    unit = lambda v: v / np.sqrt((v * v).sum(axis=-1, keepdims=True))
    fwd = unit(lookat - eye)
    right = unit(np.cross(fwd, up))
    upv = np.cross(right, fwd)
    d = unit(np.array([fwd + right * (0.9 * (i - 19.5) / 19.5) + upv * (0.6 * (j - 11.5) / 11.5) for j in range(24) for i in range(40)]))
    o = np.tile(eye, (len(d), 1))
    t, obj = _oracle.OracleScene(objs, T.Z_NEAR, T.Z_FAR, heur, T.HDRI).intersect_batch(o, d, T.Z_NEAR, T.Z_FAR, nthreads=1)
    hit = np.flatnonzero(obj >= 0)
    assert len(hit) >= N_POINTS, (name, len(hit))
    hit = hit[np.linspace(0, len(hit) - 1, N_POINTS).astype(np.int64)]
    o, d, t = o[hit], d[hit], t[hit]
    out = tuple(np.ascontiguousarray(x) for x in (o, d, o + d * t[:, None], -d))
    for x in out:
        x.setflags(write=False)
    return out


def inputs(name, kind):
    """(a, b) of a bake of the kind over the family's 130 rays or points."""
    o, d, p, nrm = geometry(name)
    return (p, nrm) if kind == "irradiance" else (o, d)


@functools.lru_cache(maxsize=None)
def point_paths(name, kind, sky, fast=False):
    """(values (130, N_MAX, 3) f64, queries (130, N_MAX) uint64): sample s of point i with index_base = 0, as the matching query
    (rayrs_scene_irradiance_mesh / rayrs_scene_radiance_mesh) runs it."""
    a, b = inputs(name, kind)
    R = reading(name, fast)
    if kind == "irradiance":
        values, queries = _mesh.irradiance_paths(R, a, b, N_MAX, BIAS, BOUNCES, SEED, lights(name, sky))
    else:
        values, queries = _mesh.radiance_paths(R, a, b, N_MAX, BOUNCES, SEED, lights(name, sky))
    return _frozen(values, queries)
