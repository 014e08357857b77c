"""The device path of the radiance queries with a mesh-light group chosen by a light tree, in a process of its own
(tests/test_gpu_tree_lights.py starts it): torch f64 tensors on the GPU, inside a side stream, answered by
rayrs_scene_radiance_mesh_launch and rayrs_scene_irradiance_mesh_launch with the light list a host array and the group a tree
handle -- equal in bits to the host path's answers after a stream sync.

Its own process because torch brings its own copy of the HIP runtime: torch must be imported BEFORE librayrs_hip.so is
loaded (as bench.py does), so that both use one runtime; in the test process the library is loaded first."""
import dataclasses
import os
import sys

import torch

torch.cuda.set_device(0)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import numpy as np  # noqa: E402

import rayrs_amd  # noqa: E402
from rayrs_amd import SKY, procedural, scenes  # noqa: E402
from rayrs_amd.api import Emission, Material  # noqa: E402


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
    objs = list(objs)
    objs[1] = dataclasses.replace(objs[1], emission=Emission.new(2.0, (1.0, 0.7, 0.5)))
    lamps = rayrs_amd.emitters(objs)
    tris = rayrs_amd.mesh_emitters(objs)[::3]
    assert len(lamps) == 1 and len(tris) >= 20
    rng = np.random.default_rng(5)
    n = 130
    o = np.tile((0.0, 5.0, 10.0), (n, 1)) + rng.normal(size=(n, 3)) * 0.1
    d = np.array((0.0, 1.0, 0.0)) - o + rng.normal(size=(n, 3)) * 1.5
    x = np.linspace(-4.0, 4.0, 9)
    p = np.array([(xi, 0.0, zi) for zi in x for xi in x])
    nrm = np.tile((0.0, 1.0, 0.0), (len(p), 1))
    kw = dict(samples=7, seed=11, index_base=5, sample_chunk=2, queries=True, direct=True)
    # the first handle's first device call is a host one, the second handle's a _launch one: each uploads the tree itself
    for first_on_device in (False, True):
        sc = rayrs_amd.Scene(objs, 1e-6, 1e6, heur, procedural.make_studio_hdri(9, 5), device=0)
        mesh, area = sc.mesh_lights(tris, tree=True), sc.mesh_lights(tris)

        def host_calls():
            return (sc.radiance(o, d, lights=lamps + [SKY], mesh=mesh, **kw), sc.radiance(o, d, fast_traversal=True, lights=lamps, mesh=mesh, **kw),
                    sc.irradiance(p, nrm, bias=1e-4, lights=[], mesh=mesh, **kw))
        host = None if first_on_device else host_calls()
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            o_d, d_d, p_d, n_d = (torch.from_numpy(a).to("cuda:0") for a in (o, d, p, nrm))
            drad = sc.radiance(o_d, d_d, lights=lamps + [SKY], mesh=mesh, **kw)
            drad_f = sc.radiance(o_d, d_d, fast_traversal=True, lights=lamps, mesh=mesh, **kw)
            dirr = sc.irradiance(p_d, n_d, bias=1e-4, lights=[], mesh=mesh, **kw)
            darea = sc.irradiance(p_d, n_d, bias=1e-4, lights=[], mesh=area, **kw)
        assert drad[0].is_cuda and tuple(drad[0].shape) == (n, 3) and drad[1].dtype == torch.uint32
        stream.synchronize()
        if host is None:
            host = host_calls()
        assert same(drad, host[0]) and same(drad_f, host[1]) and same(dirr, host[2])
        assert same(darea, sc.irradiance(p, nrm, bias=1e-4, lights=[], mesh=area, **kw))
        assert not same(darea, host[2])   # (the tree changes the answers)
        assert np.isfinite(host[0][0]).all() and np.isfinite(host[2][0]).all()
        e = torch.zeros((0, 3), dtype=torch.float64, device="cuda:0")
        assert tuple(sc.radiance(e, e, lights=[], direct=True, mesh=mesh).shape) == (0, 3)
        assert tuple(sc.irradiance(e, e, lights=[SKY], direct=True, mesh=mesh).shape) == (0, 3)
        mesh.close()
        area.close()
    print("device path ok")


if __name__ == "__main__":
    main()
