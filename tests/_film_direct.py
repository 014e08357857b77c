"""What the direct-lit films' tests (test_film_direct.py, test_gpu_film_direct.py) expect, from the plain-Python readings alone
(tests/_direct.py, tests/_sky.py): the per-sample values and closest-hit query counts of every pixel of a 20 x 12 frame -- 3 x 2
tiles, four padded columns and four padded rows: interior, right-edge, bottom-edge and corner tiles --, made once per (scene,
kernel, walk) and folded by _film.expectation, _film.noise_counts and _film_adaptive.Replay.  Nothing here calls the library
under test.

The scenes and maps are tests/test_gpu_sky.py's families: `room` (tests/_lit.py lit_room, local-pool-sized) under the studio map
with its two lamps, and `mesh1_light` (the level-1 mesh scene, which streams, has a hot group and a fast walk of its own) under the
gradient map with its lamp."""
import functools

import numpy as np

import _direct
import _lit
import _oracle
import _sky
import rayrs_amd
from rayrs_amd import procedural, scenes
from rayrs_amd.api import Material

W, H, C = 20, 12, 2
N_MAX = 9          # the longest film of the tests: passes 2 + 4 + 3
SEED, BOUNCES = 0x5EED, 50
Z_NEAR, Z_FAR = 1e-6, 1e6
MAPS = {"room": procedural.make_studio_hdri(9, 5), "mesh1_light": procedural.make_hdri(32, 16)}
KERNELS = ("direct", "sky")


@functools.lru_cache(maxsize=None)
def description(name):
    """(camera args at W x H, objects, heuristic, the map, the list's lamps) of a family."""
    if name == "room":
        cam_args, objs, heur, names = _lit.lit_room()
        lamps = (names["sphere_lamp"], names["rect_lamp"])
    else:
        cam_args, objs, heur = scenes.mesh_scene(1, Material.LambertianDiffuse((0.8, 0.8, 0.8)), area_light=True)
        lamps = tuple(rayrs_amd.emitters(objs))
    return scenes.camera_for_resolution(cam_args, W, H), objs, heur, MAPS[name], lamps


_fast_oracles = {}


def register_fast_walk(name, osc):
    """The oracle scene that walks the product's fast tree (OracleScene.use_product_walk needs the device scene: the GPU tests
    bring it)."""
    _fast_oracles[name] = osc


@functools.lru_cache(maxsize=None)
def paths(name, kernel, fast=False):
    """(rgb (H, W, N_MAX, 3) f64, queries (H, W, N_MAX) uint64) of the family's frame: sample s of pixel (row, col) as the
    kernel's image form runs it, from the reading."""
    cam_args, objs, heur, hdri, lamps = description(name)
    cls = _sky.Reading if kernel == "sky" else _direct.Reading
    R = cls(objs, Z_NEAR, Z_FAR, heur, hdri, osc=_fast_oracles[name], traversal=2) if fast else cls(objs, Z_NEAR, Z_FAR, heur, hdri)
    module = _sky if kernel == "sky" else _direct
    values, queries = module.image_paths(R, _oracle.OracleCamera(*cam_args), N_MAX, BOUNCES, SEED, lamps)
    rgb, q = values.reshape(H, W, N_MAX, 3), queries.reshape(H, W, N_MAX).astype(np.uint64)
    rgb.setflags(write=False), q.setflags(write=False)
    return rgb, q


def lights(name, kernel):
    """The list a Film (or render_lit) of the kernel takes."""
    lamps = list(description(name)[4])
    return lamps + [rayrs_amd.SKY] if kernel == "sky" else lamps
