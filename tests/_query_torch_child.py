"""The device path of the ray queries, in a process of its own (tests/test_gpu_queries.py starts it): torch f64 tensors on
the GPU, inside a side stream, answered by the _launch entry points -- bit-equal to the host path's answers after a stream
sync -- and the wrappers' refusals of tensors that are not f64, contiguous and on the scene's GPU.

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
    hit = obj != 0xFFFFFFFF
    assert hit.sum() >= 10000 and (~hit).sum() >= 10000
    t_max = np.where(np.arange(len(t)) % 2 == 0, np.nextafter(t, np.inf), t)
    occ, occ_any = sc.occluded(rays.o, rays.d, t_max), sc.occluded(rays.o, rays.d)
    assert np.array_equal(occ_any, hit) and np.array_equal(occ, hit & (np.arange(len(t)) % 2 == 0))
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        o_d, d_d, m_d = (torch.from_numpy(a).to("cuda:0") for a in (rays.o, rays.d, t_max))
        dt, dobj, dnrm = sc.intersect(o_d, d_d, normals=True)
        dt2, dobj2 = sc.intersect(o_d, d_d)
        docc, docc_any = sc.occluded(o_d, d_d, m_d), sc.occluded(o_d, d_d)
        fobj = sc.intersect(o_d, d_d, fast_traversal=True)[1]
        focc = sc.occluded(o_d, d_d, fast_traversal=True)
    for x in (dt, dobj, dnrm, dt2, dobj2, docc, docc_any, fobj, focc):
        assert x.is_cuda and x.device.index == 0
    assert dt.dtype == torch.float64 and dobj.dtype == torch.uint32 and dnrm.dtype == torch.float64 and docc.dtype == torch.bool
    assert tuple(dt.shape) == (len(t),) and tuple(dnrm.shape) == (len(t), 3) and tuple(docc.shape) == (len(t),)
    stream.synchronize()
    assert np.array_equal(bits(dt.cpu().numpy()), bits(t)) and np.array_equal(dobj.cpu().numpy(), obj)
    assert np.array_equal(bits(dnrm.cpu().numpy()), bits(nrm))
    assert np.array_equal(bits(dt2.cpu().numpy()), bits(t)) and np.array_equal(dobj2.cpu().numpy(), obj)
    assert np.array_equal(docc.cpu().numpy(), occ) and np.array_equal(docc_any.cpu().numpy(), occ_any)
    assert np.array_equal(fobj.cpu().numpy(), sc.intersect(rays.o, rays.d, fast_traversal=True)[1])
    assert np.array_equal(focc.cpu().numpy(), sc.occluded(rays.o, rays.d, fast_traversal=True))
    # none and one, on the device
    e = torch.zeros((0, 3), dtype=torch.float64, device="cuda:0")
    assert tuple(sc.intersect(e, e)[0].shape) == (0,) and tuple(sc.occluded(e, e).shape) == (0,)
    assert sc.occluded(o_d[:1], d_d[:1]).cpu().numpy().tolist() == [bool(hit[0])]
    # an f32 or CPU tensor beside a GPU tensor, a numpy array beside one, a strided one
    for bad_o, bad_d in ((o_d.float(), d_d), (o_d, d_d.cpu()), (o_d, rays.d), (o_d.t().contiguous().t(), d_d)):
        assert raises_value_error(sc.intersect, bad_o, bad_d) and raises_value_error(sc.occluded, bad_o, bad_d)
    for bad_m in (m_d.float(), m_d.cpu(), t_max, m_d[:-1]):
        assert raises_value_error(sc.occluded, o_d, d_d, bad_m)
    print("device path ok")


if __name__ == "__main__":
    main()
