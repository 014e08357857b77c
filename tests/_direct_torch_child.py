"""The device path of the direct-lighting radiance queries, in a process of its own (tests/test_gpu_direct.py starts it): torch
f64 tensors on the GPU, inside a side stream, answered by rayrs_scene_radiance_direct_launch and
rayrs_scene_irradiance_direct_launch with the light list a host array -- equal in bits to the host path's answers after a
stream sync.

Its own process because torch brings its own copy of the HIP runtime: torch must be imported BEFORE librayrs_hip.so is
loaded (as bench.py does), so that both use one runtime; in the test process the library is loaded first."""
import os
import sys

import torch

torch.cuda.set_device(0)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import numpy as np  # noqa: E402

import rayrs_amd  # noqa: E402
from rayrs_amd import procedural, scenes  # noqa: E402
from rayrs_amd.api import Material  # noqa: E402


def same(dev, host):
    for d, h in zip(dev, host):
        d = d.cpu().numpy() if torch.is_tensor(d) else d
        if h.dtype == np.float64:
            d, h = d.view(np.uint64), h.view(np.uint64)
        if not np.array_equal(d, h):
            return False
    return True


def main():
    _, objs, heur = scenes.mesh_scene(1, Material.LambertianDiffuse((0.8, 0.8, 0.8)), area_light=True)
    lights = rayrs_amd.emitters(objs)
    assert len(lights) == 1
    sc = rayrs_amd.Scene(objs, 1e-6, 1e6, heur, procedural.make_hdri(128, 64), device=0)
    rng = np.random.default_rng(5)
    n = 257
    o = np.tile((0.0, 5.0, 10.0), (n, 1)) + rng.normal(size=(n, 3)) * 0.1
    d = np.array((0.0, 1.0, 0.0)) - o + rng.normal(size=(n, 3)) * 1.5
    x = np.linspace(-4.0, 4.0, 9)
    p = np.array([(xi, 0.0, zi) for zi in x for xi in x])
    nrm = np.tile((0.0, 1.0, 0.0), (len(p), 1))
    kw = dict(samples=7, seed=11, index_base=5, sample_chunk=2, queries=True, lights=lights, direct=True)
    rad = sc.radiance(o, d, **kw)
    rad_f = sc.radiance(o, d, fast_traversal=True, **kw)
    irr = sc.irradiance(p, nrm, bias=1e-4, **kw)
    unlit = sc.radiance(o, d, **{**kw, "lights": None, "direct": False})
    lit = sc.radiance(o, d, **{**kw, "direct": False})
    assert not same(rad, unlit) and not same(rad, lit)   # (the strategy changes the answers)
    assert np.isfinite(rad[0]).all() and np.isfinite(irr[0]).all()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        o_d, d_d, p_d, n_d = (torch.from_numpy(a).to("cuda:0") for a in (o, d, p, nrm))
        drad = sc.radiance(o_d, d_d, **kw)
        drad_f = sc.radiance(o_d, d_d, fast_traversal=True, **kw)
        dirr = sc.irradiance(p_d, n_d, bias=1e-4, **kw)
        dnone = sc.radiance(o_d, d_d, **{**kw, "lights": []})
    assert drad[0].is_cuda and tuple(drad[0].shape) == (n, 3) and drad[1].dtype == torch.uint32
    stream.synchronize()
    assert same(drad, rad) and same(drad_f, rad_f) and same(dirr, irr) and same(dnone, unlit)
    e = torch.zeros((0, 3), dtype=torch.float64, device="cuda:0")
    assert tuple(sc.radiance(e, e, lights=lights, direct=True).shape) == (0, 3)
    assert tuple(sc.irradiance(e, e, lights=lights, direct=True).shape) == (0, 3)
    print("device path ok")


if __name__ == "__main__":
    main()
