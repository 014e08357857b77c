"""The device path of the radiance queries, in a process of its own (tests/test_gpu_radiance.py starts it): torch f64 tensors on
the GPU, inside a side stream, answered by rayrs_scene_radiance_launch and rayrs_scene_irradiance_launch -- bit-equal to the host
path's answers after a stream sync -- and the wrapper's refusals of tensors that are not f64, contiguous and on the scene's GPU.

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


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def raises_value_error(call, *args):
    try:
        call(*args)
    except ValueError:
        return True
    return False


def same(dev, host):
    return all(np.array_equal(bits(d.cpu().numpy()) if d.dtype == torch.float64 else d.cpu().numpy(), bits(h) if h.dtype == np.float64 else h)
               for d, h in zip(dev, host))


def main():
    _, objs, heur = scenes.mesh_scene(3, Material.LambertianDiffuse((0.8, 0.8, 0.8)), area_light=True)
    sc = rayrs_amd.Scene(objs, 1e-6, 1e6, heur, procedural.make_hdri(128, 64), device=0)
    rng = np.random.default_rng(5)
    n = 3001
    o = np.tile((0.0, 5.0, 10.0), (n, 1)) + rng.normal(size=(n, 3)) * 0.1
    d = np.array((0.0, 1.0, 0.0)) - o + rng.normal(size=(n, 3)) * 1.5
    x = np.linspace(-4.0, 4.0, 24)
    p = np.array([(xi, 0.0, zi) for zi in x for xi in x])
    nrm = np.tile((0.0, 1.0, 0.0), (len(p), 1))
    kw = dict(samples=7, seed=11, index_base=5, sample_chunk=2, queries=True)
    rad = sc.radiance(o, d, **kw)
    rad_f = sc.radiance(o, d, fast_traversal=True, **kw)
    irr = sc.irradiance(p, nrm, bias=1e-4, **kw)
    assert (rad[1] >= 14).sum() >= 500 and (rad[0] != 0.0).any(axis=1).sum() >= 2000
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        o_d, d_d, p_d, n_d = (torch.from_numpy(a).to("cuda:0") for a in (o, d, p, nrm))
        drad = sc.radiance(o_d, d_d, **kw)
        drad_f = sc.radiance(o_d, d_d, fast_traversal=True, **kw)
        dirr = sc.irradiance(p_d, n_d, bias=1e-4, **kw)
        drad_only = sc.radiance(o_d, d_d, **{**kw, "queries": False})
    for x_, m in ((drad[0], n), (drad_f[0], n), (dirr[0], len(p)), (drad_only, n)):
        assert x_.is_cuda and x_.device.index == 0 and tuple(x_.shape) == (m, 3) and x_.dtype == torch.float64
    assert drad[1].dtype == torch.uint32 and tuple(drad[1].shape) == (n,)
    stream.synchronize()
    assert same(drad, rad) and same(drad_f, rad_f) and same(dirr, irr) and same((drad_only,), rad[:1])
    # none and one, on the device
    e = torch.zeros((0, 3), dtype=torch.float64, device="cuda:0")
    assert tuple(sc.radiance(e, e).shape) == (0, 3) and tuple(sc.irradiance(e, e).shape) == (0, 3)
    one = sc.radiance(o_d[:1], d_d[:1], **kw)
    assert same(one, sc.radiance(o[:1], d[:1], **kw))
    # an f32 or CPU tensor beside a GPU tensor, a numpy array beside one, a strided one
    for bad_a, bad_b in ((o_d.float(), d_d), (o_d, d_d.cpu()), (o_d, d), (o_d.t().contiguous().t(), d_d)):
        assert raises_value_error(sc.radiance, bad_a, bad_b) and raises_value_error(sc.irradiance, bad_a, bad_b)
    print("device path ok")


if __name__ == "__main__":
    main()
