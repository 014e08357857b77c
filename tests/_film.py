"""What the progressive film's tests (test_film.py, test_gpu_film.py) expect, computed from the CPU oracle alone: the
frame from OracleScene.render(spp=N, sample_chunk=c), and the chunk sums, S1, S2 and the converged count of
include/rayrs_hip.h (NOISE) from OracleScene.path_trace_batch -- one radiance per pixel and sample index, what
path_traces(...)["rgb"] holds --
summed in numpy f64 in the stated order.  Nothing here calls the library under test."""
import functools

import numpy as np

import _oracle
from rayrs_amd import procedural, scenes
from rayrs_amd.api import Material

W, H, C, SEED, BOUNCES = 32, 24, 4, 0x5EED, 50
TAUS = (0.05, 0.2, 0.5)


def hdri():
    return procedural.make_hdri(64, 32)


def sphere_desc(w=W, h=H):
    cam_args, objs, heur = scenes.diffuse_single_sphere()
    return scenes.camera_for_resolution(cam_args, w, h), objs, heur, hdri()


def mesh_desc(w=W, h=H):
    cam_args, objs, heur = scenes.mesh_scene(3, Material.LambertianDiffuse((0.8, 0.8, 0.8)), area_light=True)
    return scenes.camera_for_resolution(cam_args, w, h), objs, heur, hdri()


DESCS = {"sphere": sphere_desc, "mesh": mesh_desc}


def oracle_of(desc):
    cam_args, objs, heur, env = desc
    return _oracle.OracleScene(objs, 1e-6, 1e6, heur, env), _oracle.OracleCamera(*cam_args)


def traces(osc, ocam, n, seed=SEED, bounces=BOUNCES):
    """rgb[row, col, s] = the radiance of sample s of the pixel, s < n, as orc_render computes it."""
    return osc.path_trace_batch(ocam, n, seed, bounces)[0]


@functools.lru_cache(maxsize=None)
def named_traces(name, n, w=W, h=H):
    osc, ocam = oracle_of(DESCS[name](w, h))
    return traces(osc, ocam, n)


def expectation(rgb, c, n):
    """The film after n samples in chunks of c, from per-sample radiance rgb[h, w, >= n, 3]: (frame, S1, S2, M).
    A chunk sum starts at +0 and takes its samples in order; the first chunk sum is assigned, later ones added in chunk
    order; S1 and S2 take the channel sums of the full chunks the same way; the frame is sum * (1 / n)."""
    h, w = rgb.shape[:2]
    total, s1, s2, m = None, np.zeros((h, w)), np.zeros((h, w)), 0
    with np.errstate(all="ignore"):
        for lo in range(0, n, c):
            hi = min(lo + c, n)
            cs = np.zeros((h, w, 3))
            for s in range(lo, hi):
                cs = cs + rgb[:, :, s]
            total = cs if total is None else total + cs
            if hi - lo == c:
                y = (cs[..., 0] + cs[..., 1]) + cs[..., 2]
                s1 = y if m == 0 else s1 + y
                s2 = y * y if m == 0 else s2 + y * y
                m += 1
        frame = total * (1.0 / float(n))
    return frame, s1, s2, m


def noise_masks(s1, s2, m, tau):
    """(unconverged, nonfinite) per pixel, by the header's predicate in its order."""
    mf = float(m)
    with np.errstate(all="ignore"):
        s11 = s1 * s1
        converged = (mf * s2 - s11 <= ((tau * tau) * s11) * (mf - 1.0)) & (m >= 2)
    nonfinite = ~(np.isfinite(s1) & np.isfinite(s2))
    return ~nonfinite & ~converged, nonfinite


def noise_counts(s1, s2, m, tau, mask=None):
    """(unconverged, nonfinite) among the pixels of mask (default: all)."""
    if mask is None:
        mask = np.ones(s1.shape, dtype=bool)
    unconverged, nonfinite = noise_masks(s1, s2, m, tau)
    return int((unconverged & mask).sum()), int((nonfinite & mask).sum())
