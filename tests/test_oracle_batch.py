"""The oracle's batched trace (orc_path_trace_batch, OracleScene.path_trace_batch), which tests/_film.py and
tests/_film_adaptive.py take their per-sample radiance and iteration counts from, held to the call it batches:
OracleScene.path_traces, one orc_path_trace per sample."""
import numpy as np
import pytest

import _film
import _film_adaptive as A
import rayrs_amd

W, H, N = 13, 11, 5   # ragged: no multiple of a tile, of the render's 16 x 16 blocks or of a thread count


@pytest.mark.parametrize("traversal", [0, 2], ids=["reference-walk", "product-walk"])
@pytest.mark.parametrize("name", sorted(_film.DESCS))
def test_the_batch_is_path_traces_bit_for_bit(name, traversal):
    desc = _film.DESCS[name](W, H)
    osc, ocam = _film.oracle_of(desc)
    assert (ocam.x_pixels(), ocam.y_pixels()) == (W, H)
    if traversal == 2:   # the product's walk on the product's tree, from a host-only scene
        _, objs, heur, env = desc
        osc.use_walk_tree(rayrs_amd.Scene(objs, 1e-6, 1e6, heur, env, device=-1), gate=True)
    pixels = [(r, c) for r in range(H) for c in range(W) for _ in range(N)]
    samples = [s for _ in range(H * W) for s in range(N)]
    one = osc.path_traces(ocam, pixels, samples, _film.SEED, _film.BOUNCES, cap=4, traversal=traversal)
    for nthreads in (1, 3, None):
        rgb, it = osc.path_trace_batch(ocam, N, _film.SEED, _film.BOUNCES, traversal=traversal, nthreads=nthreads)
        assert rgb.shape == (H, W, N, 3) and rgb.dtype == np.float64 and it.shape == (H, W, N) and it.dtype == np.uint32
        assert np.array_equal(rgb.reshape(-1, 3).view(np.uint64), np.ascontiguousarray(one["rgb"]).view(np.uint64)), nthreads
        assert np.array_equal(it.ravel(), one["n"]), nthreads
    assert len(set(one["n"].tolist())) >= 2 and one["rgb"].any()   # paths of more than one length, and light
    # the helpers' traces are the batch's
    a_rgb, a_it = A.traces(osc, ocam, N, traversal=traversal)
    assert np.array_equal(a_rgb.view(np.uint64), rgb.view(np.uint64)) and np.array_equal(a_it, it) and a_it.dtype == np.uint64
    if traversal == 0:
        assert np.array_equal(_film.traces(osc, ocam, N).view(np.uint64), rgb.view(np.uint64))
