"""The device path of ambient occlusion, in a process of its own (tests/test_gpu_ao.py starts it): torch f64 tensors on the
GPU, inside a side stream, answered by rayrs_scene_ambient_occlusion_launch -- bit-equal to the host path's answers after a
stream sync -- and the wrapper's refusals of tensors that are not f64, contiguous and on the scene's GPU.

Its own process because torch brings its own copy of the HIP runtime: torch must be imported BEFORE librayrs_hip.so is
loaded (as bench.py does), so that both use one runtime; in the test process the library is loaded first."""
import os
import sys

import torch

torch.cuda.set_device(0)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import numpy as np  # noqa: E402

import _geometry_reading as G  # noqa: E402
import rayrs_amd  # noqa: E402
from rayrs_amd import procedural  # noqa: E402


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def raises_value_error(call, *args):
    try:
        call(*args)
    except ValueError:
        return True
    return False


def main():
    rays, _ = G.scene_rays("floor_spheres")
    sc = rayrs_amd.Scene(G.SCENES["floor_spheres"](), G.T0, G.T1, G.HEURISTICS["sah1000"], procedural.make_hdri(8, 4), device=0)
    t, obj, nrm = sc.intersect(rays.o, rays.d, normals=True)
    hit = np.flatnonzero(obj != 0xFFFFFFFF)[:3001]
    p = rays.o[hit] + rays.d[hit] * t[hit][:, None]
    n = np.where((np.einsum("ij,ij->i", nrm[hit], rays.d[hit]) > 0.0)[:, None], -nrm[hit], nrm[hit])
    kw = dict(samples=7, bias=1e-3, seed=11, index_base=5)
    vis, cnt = sc.ambient_occlusion(p, n, counts=True, **kw)
    vis_r, cnt_r = sc.ambient_occlusion(p, n, counts=True, t_max=1.5, **kw)
    vis_f = sc.ambient_occlusion(p, n, fast_traversal=True, **kw)
    assert (cnt > 0).sum() >= 500 and (cnt < 7).sum() >= 500 and not np.array_equal(cnt, cnt_r)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        p_d, n_d = (torch.from_numpy(a).to("cuda:0") for a in (p, n))
        dvis, dcnt = sc.ambient_occlusion(p_d, n_d, counts=True, **kw)
        dvis_r, dcnt_r = sc.ambient_occlusion(p_d, n_d, counts=True, t_max=1.5, **kw)
        dvis_only = sc.ambient_occlusion(p_d, n_d, **kw)
        dvis_f = sc.ambient_occlusion(p_d, n_d, fast_traversal=True, **kw)
    for x in (dvis, dcnt, dvis_r, dcnt_r, dvis_only, dvis_f):
        assert x.is_cuda and x.device.index == 0 and tuple(x.shape) == (len(p),)
    assert dvis.dtype == torch.float64 and dcnt.dtype == torch.uint32
    stream.synchronize()
    assert np.array_equal(bits(dvis.cpu().numpy()), bits(vis)) and np.array_equal(dcnt.cpu().numpy(), cnt)
    assert np.array_equal(bits(dvis_r.cpu().numpy()), bits(vis_r)) and np.array_equal(dcnt_r.cpu().numpy(), cnt_r)
    assert np.array_equal(bits(dvis_only.cpu().numpy()), bits(vis)) and np.array_equal(bits(dvis_f.cpu().numpy()), bits(vis_f))
    # none and one, on the device
    e = torch.zeros((0, 3), dtype=torch.float64, device="cuda:0")
    assert tuple(sc.ambient_occlusion(e, e).shape) == (0,)
    one = sc.ambient_occlusion(p_d[:1], n_d[:1], **kw).cpu().numpy()
    assert bits(one)[0] == bits(sc.ambient_occlusion(p[:1], n[:1], **kw))[0]
    # an f32 or CPU tensor beside a GPU tensor, a numpy array beside one, a strided one
    for bad_p, bad_n in ((p_d.float(), n_d), (p_d, n_d.cpu()), (p_d, n), (p_d.t().contiguous().t(), n_d)):
        assert raises_value_error(sc.ambient_occlusion, bad_p, bad_n)
    print("device path ok")


if __name__ == "__main__":
    main()
