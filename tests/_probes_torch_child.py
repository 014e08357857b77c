"""The device path of SH probes, in a process of its own (tests/test_gpu_probes.py starts it): torch f64 points on the GPU, inside
a side stream, answered by rayrs_scene_probes_launch -- the answers stay on the device and are bit-equal to the host path's after
a stream sync, a call on a slice is the slice of the whole call there too, every lighting has its device form, a render before and
after is unchanged, sh_radiance and sh_irradiance give torch for torch, and the wrapper refuses tensors that are not f64,
contiguous and on the scene's GPU.

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
from rayrs_amd import SKY, procedural, scenes  # noqa: E402
from rayrs_amd.api import Material  # noqa: E402


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def raises_value_error(call, *args, **kw):
    try:
        call(*args, **kw)
    except ValueError:
        return True
    return False


def same(dev, host):
    return all(np.array_equal(bits(d.cpu().numpy()) if d.dtype == torch.float64 else d.cpu().numpy(), bits(h) if h.dtype == np.float64 else h)
               for d, h in zip(dev, host))


def main():
    cam_args, objs, heur = scenes.mesh_scene(3, Material.LambertianDiffuse((0.8, 0.8, 0.8)), area_light=True)
    sc = rayrs_amd.Scene(objs, 1e-6, 1e6, heur, procedural.make_hdri(128, 64), device=0)
    cam = rayrs_amd.Camera(*scenes.camera_for_resolution(cam_args, 48, 32))
    before, st0 = rayrs_amd.render(sc, cam, 4, out_f64=True)
    rng = np.random.default_rng(5)
    n = 301
    p = np.array((0.0, 1.6, 0.0)) + rng.uniform(-1.0, 1.0, size=(n, 3)) * (3.0, 1.4, 3.0)
    lamps = rayrs_amd.emitters(objs)
    kw = dict(samples=7, seed=11, index_base=5, sample_chunk=2, queries=True)
    lit = dict(lights=lamps + [SKY], direct=True)
    host = sc.probes(p, **kw)
    host_f = sc.probes(p, fast_traversal=True, **kw)
    host_lit = sc.probes(p, **kw, **lit)
    assert (host[1] >= 7).all() and (host[1] > 7).sum() >= 100 and (host[0][:, 0] > 0.0).all()
    assert not np.array_equal(bits(host[0]), bits(host_lit[0]))
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        p_d = torch.from_numpy(p).to("cuda:0")
        dev = sc.probes(p_d, **kw)
        dev_f = sc.probes(p_d, fast_traversal=True, **kw)
        dev_lit = sc.probes(p_d, **kw, **lit)
        dev_only = sc.probes(p_d, **{**kw, "queries": False})
        part = sc.probes(p_d[40:170], **{**kw, "index_base": 45})
        # the answers are evaluated where they are
        normals = torch.nn.functional.normalize(torch.from_numpy(rng.normal(size=(n, 3))).to("cuda:0"), dim=1)
        irr = rayrs_amd.sh_irradiance(dev[0], normals)
        rad = rayrs_amd.sh_radiance(dev[0], normals)
    for x_ in (dev[0], dev_f[0], dev_lit[0], dev_only):
        assert x_.is_cuda and x_.device.index == 0 and tuple(x_.shape) == (n, 9, 3) and x_.dtype == torch.float64
    assert dev[1].dtype == torch.uint32 and dev[1].is_cuda and tuple(dev[1].shape) == (n,)
    for x_ in (irr, rad):
        assert isinstance(x_, torch.Tensor) and x_.is_cuda and tuple(x_.shape) == (n, 3) and x_.dtype == torch.float64
    stream.synchronize()
    assert same(dev, host) and same(dev_f, host_f) and same(dev_lit, host_lit) and same((dev_only,), host[:1])
    assert same(part, (host[0][40:170], host[1][40:170]))
    normals_h = normals.cpu().numpy()
    assert np.allclose(irr.cpu().numpy(), rayrs_amd.sh_irradiance(host[0], normals_h), rtol=1e-13, atol=1e-15)
    assert np.allclose(rad.cpu().numpy(), rayrs_amd.sh_radiance(host[0], normals_h), rtol=1e-13, atol=1e-15)
    assert isinstance(rayrs_amd.sh_irradiance(host[0], normals_h), np.ndarray)
    # none and one, on the device
    e = torch.zeros((0, 3), dtype=torch.float64, device="cuda:0")
    assert tuple(sc.probes(e).shape) == (0, 9, 3)
    assert same(sc.probes(p_d[:1], **kw), sc.probes(p[:1], **kw))
    # an f32, a CPU or a strided tensor
    for bad in (p_d.float(), p_d.cpu(), p_d.t().contiguous().t()):
        assert raises_value_error(sc.probes, bad)
    after, st1 = rayrs_amd.render(sc, cam, 4, out_f64=True)
    assert before.tobytes() == after.tobytes() and st0["rays"] == st1["rays"] and st0["paths"] == st1["paths"]
    print("device path ok")


if __name__ == "__main__":
    main()
