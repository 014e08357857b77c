"""Host-side mirror of the rayrs-lib interface for the hot path.

Same names, argument order and error behaviour as the reference's Rust API
(paths relative to /root/reference/rayrs-lib/src):

    Material / Fresnel / Emission   material.rs:57-68, :127-131, :1056-1075
    Object::{sphere, plane, triangle, from_triangles, from_spheres, box_geom}   lib.rs:321-506
    Scene::new                      lib.rs:227
    Camera::new / x_pixels / y_pixels   lib.rs:99, :153, :175
    render(...)                     the block loop of rayrs/src/main.rs:57-101

Objects, materials and emissions are plain Python descriptions; nothing is
computed here.  Scene() hands them to librayrs_hip.so through the C ABI
(include/rayrs_hip.h), which builds the BVH and uploads it; render() runs the
gfx950 kernel.  A reference `assert!` becomes a ValueError.
"""
import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _ffi

Vec = Tuple[float, float, float]


class Axis:  # geometry.rs:161-168
    X, XRev, Y, YRev, Z, ZRev = range(6)


class BvhHeuristic:  # bvh.rs:187-191
    Midpoint = ("midpoint", 0)

    @staticmethod
    def Sah(splits: int):
        return ("sah", int(splits))


MAT_LAMBERTIAN, MAT_REFLECT, MAT_REFRACT, MAT_GLASS, MAT_COOK_TORRANCE, MAT_COOK_TORRANCE_REFRACT, \
    MAT_COOK_TORRANCE_GLASS, MAT_PLASTIC, MAT_NO_REFLECT = range(9)


def _v(x) -> Vec:
    a = tuple(float(c) for c in x)
    if len(a) != 3:
        raise ValueError("expected 3 components")
    return a


@dataclass(frozen=True)
class Fresnel:  # material.rs:127-131
    metallic: bool
    ior: float = 0.0
    r0: Vec = (0.0, 0.0, 0.0)

    @staticmethod
    def SchlickDielectric(ior: float) -> "Fresnel":
        return Fresnel(False, float(ior))

    @staticmethod
    def SchlickMetallic(r0) -> "Fresnel":
        return Fresnel(True, 0.0, _v(r0))


@dataclass(frozen=True)
class Material:  # material.rs:57-68
    kind: int
    color: Vec = (0.0, 0.0, 0.0)
    spec_color: Vec = (0.0, 0.0, 0.0)
    alpha: float = 0.0
    ior: float = 0.0
    metallic: bool = False
    r0: Vec = (0.0, 0.0, 0.0)

    # constructors, in the reference's argument order
    @staticmethod
    def LambertianDiffuse(color) -> "Material":  # material.rs:608
        return Material(MAT_LAMBERTIAN, _v(color))

    @staticmethod
    def Reflect(color) -> "Material":  # :629
        return Material(MAT_REFLECT, _v(color))

    @staticmethod
    def Refract(color, ior) -> "Material":  # :650
        return Material(MAT_REFRACT, _v(color), ior=float(ior))

    @staticmethod
    def Glass(color, ior) -> "Material":  # :673
        return Material(MAT_GLASS, _v(color), ior=float(ior))

    @staticmethod
    def CookTorrance(color, alpha, fresnel: Fresnel) -> "Material":  # :705
        return Material(MAT_COOK_TORRANCE, _v(color), alpha=float(alpha), ior=fresnel.ior,
                        metallic=fresnel.metallic, r0=fresnel.r0)

    @staticmethod
    def CookTorranceRefract(color, alpha, ior) -> "Material":  # :832
        return Material(MAT_COOK_TORRANCE_REFRACT, _v(color), alpha=float(alpha), ior=float(ior))

    @staticmethod
    def CookTorranceGlass(color, alpha, ior) -> "Material":  # :863
        return Material(MAT_COOK_TORRANCE_GLASS, _v(color), alpha=float(alpha), ior=float(ior))

    @staticmethod
    def Plastic(color, spec_color, alpha, ior) -> "Material":  # :887
        return Material(MAT_PLASTIC, _v(color), _v(spec_color), float(alpha), float(ior))

    @staticmethod
    def NoReflect() -> "Material":
        return Material(MAT_NO_REFLECT)

    def desc(self) -> _ffi.MaterialDesc:
        d = _ffi.MaterialDesc()
        d.kind = self.kind
        d.metallic = 1 if self.metallic else 0
        d.color[:] = self.color
        d.spec_color[:] = self.spec_color
        d.alpha = self.alpha
        d.ior = self.ior
        d.r0[:] = self.r0
        return d


@dataclass(frozen=True)
class Emission:  # material.rs:1056-1075
    emissive: bool = False
    strength: float = 0.0
    color: Vec = (0.0, 0.0, 0.0)

    @staticmethod
    def Dark() -> "Emission":
        return Emission()

    @staticmethod
    def new(strength, color) -> "Emission":  # Emission::new, :1067
        return Emission(True, float(strength), _v(color))

    Emissive = new

    def desc(self) -> _ffi.EmissionDesc:
        d = _ffi.EmissionDesc()
        d.emissive = 1 if self.emissive else 0
        d.strength = self.strength
        d.color[:] = self.color
        return d


@dataclass
class Object:  # lib.rs:302-306
    """One scene object, or (kind == "mesh") the Vec<Object> that
    Object::from_triangles returns for an indexed triangle mesh."""
    kind: str
    mat: Material
    emission: Emission
    radius: float = 0.0
    origin: Vec = (0.0, 0.0, 0.0)
    axis: int = 0
    umin: float = 0.0
    umax: float = 0.0
    vmin: float = 0.0
    vmax: float = 0.0
    pos: float = 0.0
    p: Tuple[Vec, Vec, Vec] = ((0, 0, 0),) * 3
    verts: Optional[np.ndarray] = field(default=None, repr=False)  # (n,3) f32 or f64
    idx: Optional[np.ndarray] = field(default=None, repr=False)    # (m,3) u32

    @staticmethod
    def sphere(radius, origin, mat, emission) -> "Object":  # lib.rs:321
        return Object("sphere", mat, emission, radius=float(radius), origin=_v(origin))

    @staticmethod
    def plane(axis, umin, umax, vmin, vmax, pos, mat, emission) -> "Object":  # lib.rs:342
        return Object("plane", mat, emission, axis=int(axis), umin=float(umin), umax=float(umax),
                      vmin=float(vmin), vmax=float(vmax), pos=float(pos))

    @staticmethod
    def triangle(p1, p2, p3, mat, emission) -> "Object":  # lib.rs:380
        return Object("triangle", mat, emission, p=(_v(p1), _v(p2), _v(p3)))

    @staticmethod
    def from_triangles(verts, idx, mat, emission) -> List["Object"]:  # lib.rs:407
        verts = np.ascontiguousarray(verts)
        if verts.dtype not in (np.float32, np.float64):
            verts = verts.astype(np.float64)
        idx = np.ascontiguousarray(idx, dtype=np.uint32)
        if verts.ndim != 2 or verts.shape[1] != 3 or idx.ndim != 2 or idx.shape[1] != 3:
            raise ValueError("verts must be (n,3) and idx (m,3)")
        return [Object("mesh", mat, emission, verts=verts, idx=idx)]

    @staticmethod
    def from_spheres(radius, centers, mat, emission) -> List["Object"]:  # lib.rs:422
        return [Object.sphere(radius, c, mat, emission) for c in np.asarray(centers, dtype=np.float64)]

    @staticmethod
    def box_geom(lower_left, upper_right, mat, emission) -> List["Object"]:  # lib.rs:438-506
        ll, ur = _v(lower_left), _v(upper_right)
        return [
            Object.plane(Axis.X, ll[1], ur[1], ll[2], ur[2], ll[0], mat, emission),
            Object.plane(Axis.XRev, ll[1], ur[1], ll[2], ur[2], ur[0], mat, emission),
            Object.plane(Axis.ZRev, ll[0], ur[0], ll[1], ur[1], ll[2], mat, emission),
            Object.plane(Axis.Z, ll[0], ur[0], ll[1], ur[1], ur[2], mat, emission),
            Object.plane(Axis.YRev, ll[0], ur[0], ll[2], ur[2], ll[1], mat, emission),
            Object.plane(Axis.Y, ll[0], ur[0], ll[2], ur[2], ll[1], mat, emission),
        ]


def _d3(v):
    return (C.c_double * 3)(*v)


def _is_torch(a) -> bool:
    """A torch tensor, told without importing torch where nobody uses it."""
    return type(a).__module__.split(".")[0] == "torch"


def flatten_objects(objects) -> List[Object]:
    out = []
    for o in objects:
        if isinstance(o, (list, tuple)):
            out.extend(flatten_objects(o))
        else:
            out.append(o)
    return out


class Camera:
    """Pinhole camera, lib.rs:54-211."""

    def __init__(self, origin, up, lookat, fov, width, height, ppi):
        L = _ffi.lib()
        self.args = (_v(origin), _v(up), _v(lookat), float(fov), float(width), float(height), int(ppi))
        self.desc = _ffi.CameraDesc()
        st = L.rayrs_camera_new(_d3(self.args[0]), _d3(self.args[1]), _d3(self.args[2]), self.args[3],
                                self.args[4], self.args[5], self.args[6], C.byref(self.desc))
        if st == -1:
            raise ValueError("Camera::new: invalid argument (lib.rs:108-111)")
        _ffi.check(st, "rayrs_camera_new")

    def x_pixels(self) -> int:  # lib.rs:153
        return int(self.desc.x_pixels)

    def y_pixels(self) -> int:  # lib.rs:175
        return int(self.desc.y_pixels)


class Scene:
    """Scene::new(objects, z_near, z_far, heuristic, hdri), lib.rs:227.

    hdri: (H, W, 3) float32 array (what image::hdr::HdrDecoder yields at
    main.rs:36-41); it is clipped to [0, 3] inside the library as main.rs:43
    does.  device = -1 builds a host-only scene (BVH inspection, no render).
    """

    def __init__(self, objects, z_near, z_far, heuristic, hdri, device: int = 0):
        L = _ffi.lib()
        self._L = L
        self._h = None
        objs = C.c_void_p()
        _ffi.check(L.rayrs_objects_create(C.byref(objs)), "rayrs_objects_create")
        try:
            for o in flatten_objects(objects):
                m, e = o.mat.desc(), o.emission.desc()
                if o.kind == "sphere":
                    st = L.rayrs_object_sphere(objs, o.radius, _d3(o.origin), C.byref(m), C.byref(e))
                elif o.kind == "plane":
                    st = L.rayrs_object_plane(objs, o.axis, o.umin, o.umax, o.vmin, o.vmax, o.pos, C.byref(m),
                                              C.byref(e))
                elif o.kind == "triangle":
                    st = L.rayrs_object_triangle(objs, _d3(o.p[0]), _d3(o.p[1]), _d3(o.p[2]), C.byref(m),
                                                 C.byref(e))
                elif o.kind == "mesh":
                    fn = (L.rayrs_object_from_triangles_f32 if o.verts.dtype == np.float32
                          else L.rayrs_object_from_triangles_f64)
                    st = fn(objs, o.verts.ctypes.data, o.verts.shape[0], o.idx.ctypes.data, o.idx.shape[0],
                            C.byref(m), C.byref(e))
                else:
                    raise ValueError(f"unknown object kind {o.kind}")
                if st == -1:
                    raise ValueError(f"Object::{o.kind}: invalid argument (a reference assert! would fire)")
                _ffi.check(st, f"rayrs_object_{o.kind}")
            hdri = np.ascontiguousarray(hdri, dtype=np.float32)
            if hdri.ndim != 3 or hdri.shape[2] != 3:
                raise ValueError("hdri must be (H, W, 3)")
            kind, splits = heuristic
            h = C.c_void_p()
            st = L.rayrs_scene_new(objs, float(z_near), float(z_far), 1 if kind == "sah" else 0, int(splits),
                                   hdri.shape[1], hdri.shape[0], hdri.ctypes.data, int(device), C.byref(h))
            if st == -1:
                raise ValueError("Scene::new: invalid argument (lib.rs:234-235, bvh.rs:229)")
            _ffi.check(st, "rayrs_scene_new")
            self._h = h
            self.device = int(device)
            self._hdri_size = (int(hdri.shape[1]), int(hdri.shape[0]))
        finally:
            L.rayrs_objects_destroy(objs)

    @classmethod
    def _from_handle(cls, L, h, device):
        self = cls.__new__(cls)
        self._L, self._h, self.device = L, h, int(device)
        return self

    def clone_to_device(self, device: int) -> "Scene":
        """The same scene uploaded to another HIP device without building the BVH again
        (one per GPU for render_multi)."""
        h = C.c_void_p()
        _ffi.check(self._L.rayrs_scene_clone_to_device(self._h, int(device), C.byref(h)), "rayrs_scene_clone_to_device")
        clone = Scene._from_handle(self._L, h, device)
        clone._hdri_size = self._hdri_size
        return clone

    def set_tuning(self, **kw):
        """The two scheduling choices of include/rayrs_hip.h rayrs_tuning (pool_slots, local_pool); 0 = default.
        They do not change the arithmetic (the routes differ in which primitives a query tests: include/rayrs_hip.h)."""
        t = _ffi.Tuning()
        for k, v in kw.items():
            if k not in dict(_ffi.Tuning._fields_):
                raise ValueError(f"unknown tuning field {k}")
            setattr(t, k, int(v))
        _ffi.check(self._L.rayrs_scene_set_tuning(self._h, C.byref(t)), "rayrs_scene_set_tuning")

    def lab_set(self, **kw):
        """The kernels' development knobs (rayrs_amd/csrc/rayrs_lab.h): for tests and scripts/ubench only."""
        t = _ffi.LabTuning()
        for k, v in kw.items():
            if k not in dict(_ffi.LabTuning._fields_):
                raise ValueError(f"unknown lab field {k}")
            setattr(t, k, int(v))
        _ffi.check(self._L.rayrs_lab_set(self._h, C.byref(t)), "rayrs_lab_set")

    def lab_stack_need(self, which: int) -> int:
        """rayrs_amd/csrc/rayrs_lab.h rayrs_lab_stack_need: the entries of a lane's stack on tree 0 (fast walk), 1 (gate), 2 (gate
        without the hot group); for tests only."""
        n = self._L.rayrs_lab_stack_need(self._h, int(which))
        if n < 0:
            _ffi.check(n, "rayrs_lab_stack_need")
        return int(n)

    def info(self) -> dict:
        i = _ffi.SceneInfo()
        _ffi.check(self._L.rayrs_scene_info(self._h, C.byref(i)), "rayrs_scene_info")
        d = {n: getattr(i, n) for n, _ in i._fields_ if n not in ("root_box", "hot_box")}
        d["root_box"] = list(i.root_box)
        d["hot_box"] = list(i.hot_box)
        return d

    def export_bvh(self):
        i = self.info()
        box = np.zeros((max(i["n_interior"], 1), 2, 6), dtype=np.float64)
        ref = np.zeros((max(i["n_interior"], 1), 2), dtype=np.uint32)
        prim = np.zeros(max(i["n_prims"], 1), dtype=np.uint32)
        _ffi.check(self._L.rayrs_scene_export_bvh(self._h, box.ctypes.data, ref.ctypes.data, prim.ctypes.data),
                   "rayrs_scene_export_bvh")
        return box[:i["n_interior"]], ref[:i["n_interior"]], prim[:i["n_prims"]]

    def export_wide(self):
        """The four-slot records the fast walk reads: (box[n_wide,4,6], ref[n_wide,4])."""
        i = self.info()
        box = np.zeros((max(i["n_wide"], 1), 4, 6), dtype=np.float64)
        ref = np.zeros((max(i["n_wide"], 1), 4), dtype=np.uint32)
        _ffi.check(self._L.rayrs_scene_export_wide(self._h, box.ctypes.data, ref.ctypes.data),
                   "rayrs_scene_export_wide")
        return box[:i["n_wide"]], ref[:i["n_wide"]]

    def export_gate_tree(self):
        """The records the default walk reads (the reference's leaf groups behind their gating boxes):
        (box[gate_n_wide,4,6], ref[gate_n_wide,4])."""
        i = self.info()
        box = np.zeros((max(i["gate_n_wide"], 1), 4, 6), dtype=np.float64)
        ref = np.zeros((max(i["gate_n_wide"], 1), 4), dtype=np.uint32)
        _ffi.check(self._L.rayrs_scene_export_gate_tree(self._h, box.ctypes.data, ref.ctypes.data),
                   "rayrs_scene_export_gate_tree")
        return box[:i["gate_n_wide"]], ref[:i["gate_n_wide"]]

    def export_hot_tree(self):
        """The gate tree without the scene's hot group (info()["hot_count"] > 0): what the default walk reads there:
        (box[hot_n_wide,4,6], ref[hot_n_wide,4])."""
        i = self.info()
        box = np.zeros((max(i["hot_n_wide"], 1), 4, 6), dtype=np.float64)
        ref = np.zeros((max(i["hot_n_wide"], 1), 4), dtype=np.uint32)
        _ffi.check(self._L.rayrs_scene_export_hot_tree(self._h, box.ctypes.data, ref.ctypes.data),
                   "rayrs_scene_export_hot_tree")
        return box[:i["hot_n_wide"]], ref[:i["hot_n_wide"]]

    # ---- ray queries (include/rayrs_hip.h RAY QUERIES)

    def _query_inputs(self, origins, directions, t_max=None):
        """The rays of a query, checked before any library call: (torch module or None, origins, directions, t_max, n).
        numpy inputs become contiguous f64 arrays; torch tensors are taken as they are and must be f64, contiguous and on the
        scene's GPU, all of them."""
        given = [a for a in (origins, directions, t_max) if a is not None]
        if any(_is_torch(a) for a in given):
            import torch
            for a in given:
                if not _is_torch(a) or a.dtype != torch.float64 or not a.is_cuda or a.device.index != self.device \
                        or not a.is_contiguous():
                    raise ValueError(f"a query on device tensors takes contiguous float64 tensors on cuda:{self.device}, all of them")
        else:
            torch = None
            origins, directions = (np.ascontiguousarray(a, dtype=np.float64) for a in (origins, directions))
            t_max = None if t_max is None else np.ascontiguousarray(t_max, dtype=np.float64)
        for a in (origins, directions):
            if a.ndim != 2 or a.shape[1] != 3:
                raise ValueError("origins and directions must be (n, 3)")
        n = int(origins.shape[0])
        if int(directions.shape[0]) != n:
            raise ValueError("origins and directions must have the same length")
        if t_max is not None and tuple(t_max.shape) != (n,):
            raise ValueError(f"t_max must be ({n},)")
        return torch, origins, directions, t_max, n

    def intersect(self, origins, directions, fast_traversal: bool = False, normals: bool = False):
        """The closest hit of every ray (origins[i], directions[i]), the render's query: (t, object) or, with normals,
        (t, object, normal) -- t (n,) f64, object (n,) uint32 in insertion order (0xFFFFFFFF: a miss, t and normal then 0),
        normal (n, 3) f64, not flipped.  (n, 3) numpy arrays are answered through host buffers and return numpy; f64 torch
        tensors on the scene's GPU are answered on torch's current stream and return tensors there, nothing copied to the
        host and no wait.  (For the device path import torch before the library is first used -- before the first Scene or
        Camera -- as bench.py does: torch brings its own copy of the HIP runtime, and only a library loaded after it shares
        torch's; loaded first, the process has two runtimes and torch finds no device.)"""
        torch, o, d, _, n = self._query_inputs(origins, directions)
        m = max(n, 1)  # (an empty batch still hands the library buffers)
        if torch is None:
            t, obj = np.zeros(m), np.zeros(m, dtype=np.uint32)
            nrm = np.zeros((m, 3)) if normals else None
            o, d = (a if n else np.zeros((1, 3)) for a in (o, d))
            _ffi.check(self._L.rayrs_scene_intersect(self._h, o.ctypes.data, d.ctypes.data, n, int(bool(fast_traversal)),
                                                     t.ctypes.data, obj.ctypes.data, _ptr(nrm)), "rayrs_scene_intersect")
        else:
            dev = o.device
            t = torch.empty(m, dtype=torch.float64, device=dev)
            obj = torch.empty(m, dtype=torch.int32, device=dev).view(torch.uint32)
            nrm = torch.empty((m, 3), dtype=torch.float64, device=dev) if normals else None
            o, d = (a if n else torch.zeros((1, 3), dtype=torch.float64, device=dev) for a in (o, d))
            _ffi.check(self._L.rayrs_scene_intersect_launch(self._h, o.data_ptr(), d.data_ptr(), n, int(bool(fast_traversal)),
                                                            t.data_ptr(), obj.data_ptr(), None if nrm is None else nrm.data_ptr(),
                                                            torch.cuda.current_stream(dev).cuda_stream),
                       "rayrs_scene_intersect_launch")
        return (t[:n], obj[:n], nrm[:n]) if normals else (t[:n], obj[:n])

    def occluded(self, origins, directions, t_max=None, fast_traversal: bool = False):
        """Whether the closest hit of every ray lies before t_max[i] (None: anywhere), as a bool array: an any-hit walk that
        stops at the first accepted hit with t < t_max.  A NaN, zero or negative t_max gives False.  Inputs and where the
        answer lives as intersect()."""
        torch, o, d, tm, n = self._query_inputs(origins, directions, t_max)
        m = max(n, 1)
        if torch is None:
            occ = np.zeros(m, dtype=np.uint8)
            o, d = (a if n else np.zeros((1, 3)) for a in (o, d))
            _ffi.check(self._L.rayrs_scene_occluded(self._h, o.ctypes.data, d.ctypes.data, _ptr(tm) if n else None, n,
                                                    int(bool(fast_traversal)), occ.ctypes.data), "rayrs_scene_occluded")
            return occ[:n].astype(bool)
        dev = o.device
        occ = torch.empty(m, dtype=torch.uint8, device=dev)
        o, d = (a if n else torch.zeros((1, 3), dtype=torch.float64, device=dev) for a in (o, d))
        _ffi.check(self._L.rayrs_scene_occluded_launch(self._h, o.data_ptr(), d.data_ptr(), tm.data_ptr() if tm is not None and n else None,
                                                       n, int(bool(fast_traversal)), occ.data_ptr(),
                                                       torch.cuda.current_stream(dev).cuda_stream), "rayrs_scene_occluded_launch")
        return occ[:n].view(torch.bool)

    # ---- ambient occlusion (include/rayrs_hip.h AMBIENT OCCLUSION)

    def ambient_occlusion(self, points, normals, samples: int = 16, t_max=None, bias: float = 0.0, seed: int = 0x5EED,
                          index_base: int = 0, fast_traversal: bool = False, counts: bool = False):
        """The share of `samples` cosine-distributed rays around normals[i], leaving points[i] + normals[i] * bias, that
        reach t_max (None: anywhere) unoccluded: visibility (n,) f64, and with counts also the occluded samples per point,
        (n,) uint32.  Points and normals are used as given.  A call on points[a:b] with index_base=a returns the slice of the
        whole call's answer.  Inputs and where the answers live as intersect()."""
        torch, p, nrm, _, n = self._query_inputs(points, normals)
        if int(samples) < 1:
            raise ValueError("samples must be at least 1")
        m = max(n, 1)
        args = (n, int(samples), float("inf") if t_max is None else float(t_max), float(bias), int(seed), int(index_base),
                int(bool(fast_traversal)))
        if torch is None:
            cnt, vis = np.zeros(m, dtype=np.uint32), np.zeros(m)
            p, nrm = (a if n else np.zeros((1, 3)) for a in (p, nrm))
            _ffi.check(self._L.rayrs_scene_ambient_occlusion(self._h, p.ctypes.data, nrm.ctypes.data, *args, cnt.ctypes.data,
                                                             vis.ctypes.data), "rayrs_scene_ambient_occlusion")
        else:
            dev = p.device
            cnt = torch.empty(m, dtype=torch.int32, device=dev).view(torch.uint32)
            vis = torch.empty(m, dtype=torch.float64, device=dev)
            p, nrm = (a if n else torch.zeros((1, 3), dtype=torch.float64, device=dev) for a in (p, nrm))
            _ffi.check(self._L.rayrs_scene_ambient_occlusion_launch(self._h, p.data_ptr(), nrm.data_ptr(), *args, cnt.data_ptr(),
                                                                    vis.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
                       "rayrs_scene_ambient_occlusion_launch")
        return (vis[:n], cnt[:n]) if counts else vis[:n]

    def lab_ao_refill(self, refill_below: int = 0):
        """rayrs_amd/csrc/rayrs_lab.h rayrs_lab_ao_refill: for tests and scripts/ubench only; 0 = the default."""
        _ffi.check(self._L.rayrs_lab_ao_refill(self._h, int(refill_below)), "rayrs_lab_ao_refill")

    # ---- radiance queries (include/rayrs_hip.h RADIANCE QUERY, IRRADIANCE)

    def _radiance(self, name, a, b, samples, max_bounces, sample_chunk, bias, seed, index_base, fast_traversal, queries, lights=None,
                  direct=False, mesh=None):
        if direct and lights is None:
            raise ValueError("direct=True needs a light list (lights=[...])")
        if mesh is not None and not direct:
            raise ValueError("mesh=... needs direct=True (a mesh-light group is a light of direct lighting)")
        torch, a, b, _, n = self._query_inputs(a, b)
        if int(samples) < 1:
            raise ValueError("samples must be at least 1")
        m = max(n, 1)
        args = (n, int(samples), int(max_bounces), int(sample_chunk)) + (() if bias is None else (float(bias),)) + \
               (int(seed), int(index_base), int(bool(fast_traversal)))
        if lights is not None:  # (a host array in every form: include/rayrs_hip.h LIGHT SAMPLING)
            lights = _light_list(lights)
            sky = bool(direct) and bool((lights == SKY).any())   # (SKY SAMPLING: the sky beside the lamps, named once or often)
            if sky:
                lights = lights[lights != SKY]
            name += "_mesh" if mesh is not None else "_sky" if sky else "_direct" if direct else "_lit"
            args += (lights.ctypes.data if len(lights) else None, len(lights))
            if mesh is not None:  # (MESH LIGHTS: the group and the sky as arguments of their own)
                args += (mesh._handle(), int(sky))
        if torch is None:
            rad, cnt = np.zeros((m, 3)), np.zeros(m, dtype=np.uint32)
            a, b = (x if n else np.zeros((1, 3)) for x in (a, b))
            _ffi.check(getattr(self._L, name)(self._h, a.ctypes.data, b.ctypes.data, *args, rad.ctypes.data, cnt.ctypes.data), name)
        else:
            dev = a.device
            rad = torch.empty((m, 3), dtype=torch.float64, device=dev)
            cnt = torch.empty(m, dtype=torch.int32, device=dev).view(torch.uint32)
            a, b = (x if n else torch.zeros((1, 3), dtype=torch.float64, device=dev) for x in (a, b))
            _ffi.check(getattr(self._L, name + "_launch")(self._h, a.data_ptr(), b.data_ptr(), *args, rad.data_ptr(), cnt.data_ptr(),
                                                          torch.cuda.current_stream(dev).cuda_stream), name + "_launch")
        return (rad[:n], cnt[:n]) if queries else rad[:n]

    def radiance(self, origins, directions, samples: int = 1, max_bounces: int = 50, seed: int = 0x5EED, index_base: int = 0,
                 sample_chunk: int = 0, fast_traversal: bool = False, queries: bool = False, lights=None,
                 mesh: Optional["MeshLights"] = None, direct: bool = False):
        """The path-traced light arriving along every ray (origins[i], directions[i]), the mean of `samples` paths of the
        render's radiance loop: radiance (n, 3) f64, and with queries also the number of closest-hit queries the ray's paths
        made, (n,) uint32.  Rays are used as given.  Sample s of ray i draws from the key of (seed, index_base + i, s), so a
        call on rays[a:b] with index_base=a returns the slice of the whole call's answer; sample_chunk is
        rayrs_render_params.sample_chunk's rule for the order of the sum.  lights: None, or up to 8 object indices (emitters())
        that diffuse surfaces sample half of the time (include/rayrs_hip.h LIGHT SAMPLING; an empty list computes what None
        computes).  direct=True (with lights): every diffuse bounce keeps its own direction and sends one more ray towards a
        sampled point of a light, the two weighted by the balance heuristic (include/rayrs_hip.h DIRECT LIGHTING); with SKY in
        the list the environment map is one more of those lights, its directions drawn in proportion to its brightness
        (include/rayrs_hip.h SKY SAMPLING; lights=[SKY] is the sky alone).  mesh (with direct=True): a group of emissive
        triangles of this scene (mesh_lights()) as one more of those lights, its points drawn uniformly by area
        (include/rayrs_hip.h MESH LIGHTS; lights may then be empty).  Inputs and where the answers live as intersect()."""
        return self._radiance("rayrs_scene_radiance", origins, directions, samples, max_bounces, sample_chunk, None, seed, index_base,
                              fast_traversal, queries, lights, direct, mesh)

    def irradiance(self, points, normals, samples: int = 64, bias: float = 0.0, max_bounces: int = 50, seed: int = 0x5EED,
                   index_base: int = 0, sample_chunk: int = 0, fast_traversal: bool = False, queries: bool = False, lights=None,
                   mesh: Optional["MeshLights"] = None, direct: bool = False):
        """The cosine-weighted mean of the light arriving at points[i] around normals[i], E / pi, from `samples` paths that
        leave points[i] + normals[i] * bias in ambient_occlusion()'s directions: (n, 3) f64 (multiply by pi for the
        irradiance; a Lambertian texel of albedo rho radiates rho times the value).  Points and normals are used as given.
        With lights the first direction too is drawn from the mix of the lights and the cosine lobe, and the sample is weighted
        for it: the same mean, with less noise under a small lamp.  With direct=True the first direction stays the cosine lobe's
        and the point sends a shadow ray of its own, as a diffuse bounce does.  The other arguments, inputs and answers as
        radiance()."""
        return self._radiance("rayrs_scene_irradiance", points, normals, samples, max_bounces, sample_chunk, bias, seed, index_base,
                              fast_traversal, queries, lights, direct, mesh)

    # ---- SH probes (include/rayrs_hip.h SH PROBES)

    def probes(self, points, samples: int = 256, max_bounces: int = 50, seed: int = 0x5EED, index_base: int = 0, sample_chunk: int = 0,
               fast_traversal: bool = False, queries: bool = False, lights=None, direct: bool = False,
               mesh: Optional["MeshLights"] = None):
        """The light arriving at every point from all directions, projected onto the nine real spherical harmonics of orders
        0 to 2 per colour channel: coeffs (n, 9, 3) f64 in the order (l, m) = (0,0), (1,-1), (1,0), (1,1), (2,-2) .. (2,2) on
        the scene's own axes, and with queries also the closest-hit queries of the probe's paths, (n,) uint32.  Each of the
        `samples` paths of probe i leaves points[i] in a direction drawn uniformly over the sphere from the key of (seed,
        index_base + i, s), so a call on points[a:b] with index_base=a returns the slice of the whole call's answer;
        sample_chunk is radiance()'s rule for the order of the sums.  lights (with direct=True), SKY among them, and mesh (with
        direct=True) are radiance()'s: the paths are then the direct-lit ones, a tree group included; lights=None and lights=[]
        are the unlit paths.  A list without direct=True is refused: the one-sample mix has no probes.  sh_radiance() and
        sh_irradiance() evaluate the answer.  (n, 3) numpy points go through host buffers; float64 tensors on the scene's GPU
        are answered on torch's current stream and stay on the device."""
        if lights is not None and len(lights) and not direct:
            raise ValueError("probes with a light list need direct=True (the one-sample mix has no probes)")
        if mesh is not None and not direct:
            raise ValueError("mesh=... needs direct=True (a mesh-light group is a light of direct lighting)")
        if int(samples) < 1:
            raise ValueError("samples must be at least 1")
        if _is_torch(points):
            import torch
            if points.dtype != torch.float64 or not points.is_cuda or points.device.index != self.device or not points.is_contiguous():
                raise ValueError(f"probes on a device tensor take a contiguous float64 tensor on cuda:{self.device}")
        else:
            torch = None
            points = np.ascontiguousarray(points, dtype=np.float64)
        if points.ndim != 2 or points.shape[1] != 3:
            raise ValueError("points must be (n, 3)")
        n = int(points.shape[0])
        m = max(n, 1)
        lights = _light_list([] if lights is None else lights)
        sky = bool((lights == SKY).any())
        lights = lights[lights != SKY]
        args = (n, int(samples), int(max_bounces), int(sample_chunk), int(seed), int(index_base), int(bool(fast_traversal)),
                lights.ctypes.data if len(lights) else None, len(lights), None if mesh is None else mesh._handle(), int(sky))
        if torch is None:
            coeffs, cnt = np.zeros((m, 9, 3)), np.zeros(m, dtype=np.uint32)
            pts = points if n else np.zeros((1, 3))
            _ffi.check(self._L.rayrs_scene_probes(self._h, pts.ctypes.data, *args, coeffs.ctypes.data, cnt.ctypes.data), "rayrs_scene_probes")
        else:
            dev = points.device
            coeffs = torch.empty((m, 9, 3), dtype=torch.float64, device=dev)
            cnt = torch.empty(m, dtype=torch.int32, device=dev).view(torch.uint32)
            pts = points if n else torch.zeros((1, 3), dtype=torch.float64, device=dev)
            _ffi.check(self._L.rayrs_scene_probes_launch(self._h, pts.data_ptr(), *args, coeffs.data_ptr(), cnt.data_ptr(),
                                                         torch.cuda.current_stream(dev).cuda_stream), "rayrs_scene_probes_launch")
        return (coeffs[:n], cnt[:n]) if queries else coeffs[:n]

    # ---- a mesh-light group (include/rayrs_hip.h MESH LIGHTS)

    def mesh_lights(self, tris, tree: bool = False) -> "MeshLights":
        """A mesh-light group of this scene: `tris` are the object indices of its triangles (mesh_emitters()), each at most
        once.  What radiance(), irradiance() and render_lit() take as mesh=...; close it before the scene.  tree=True: the
        group's triangle is chosen per shading point by a light tree, by power over squared distance (include/rayrs_hip.h LIGHT
        TREE), instead of uniformly by area; films and bakes do not take such a group."""
        return MeshLights(self, tris, tree)

    # ---- the sky as a light (include/rayrs_hip.h SKY SAMPLING): host only, a scene without a device has them too

    def sky_table(self):
        """The sky's table: (cells (h - 1, w - 1) f64 -- A[i][j], the weight of bilinear cell (i, j) of the HDRI --, their total T)."""
        w, h = self._hdri_size
        cells, total = np.zeros((h - 1, w - 1)), C.c_double()
        _ffi.check(self._L.rayrs_scene_sky_table(self._h, cells.ctypes.data, C.addressof(total)), "rayrs_scene_sky_table")
        return cells, total.value

    def sky_sample(self, u):
        """sky_sample(u1, u2) of every row of u (n, 2): directions (n, 3) f64, distributed in proportion to the HDRI's brightness."""
        u = np.ascontiguousarray(u, dtype=np.float64)
        if u.ndim != 2 or u.shape[1] != 2:
            raise ValueError("u must be (n, 2)")
        out = np.zeros((max(len(u), 1), 3))
        _ffi.check(self._L.rayrs_scene_sky_sample(self._h, u.ctypes.data if len(u) else out.ctypes.data, len(u), out.ctypes.data),
                   "rayrs_scene_sky_sample")
        return out[:len(u)]

    def sky_density(self, directions):
        """p_env of every direction (n, 3): the solid-angle density of sky_sample's directions, (n,) f64."""
        d = np.ascontiguousarray(directions, dtype=np.float64)
        if d.ndim != 2 or d.shape[1] != 3:
            raise ValueError("directions must be (n, 3)")
        out = np.zeros(max(len(d), 1))
        _ffi.check(self._L.rayrs_scene_sky_density(self._h, d.ctypes.data if len(d) else out.ctypes.data, len(d), out.ctypes.data),
                   "rayrs_scene_sky_density")
        return out[:len(d)]

    def lab_radiance_tuning(self, refill_below: int = 0, shade_at: int = 0, leaf_min: int = 0):
        """rayrs_amd/csrc/rayrs_lab.h rayrs_lab_radiance_tuning: for tests and scripts/ubench only; 0 = the default."""
        _ffi.check(self._L.rayrs_lab_radiance_tuning(self._h, int(refill_below), int(shade_at), int(leaf_min)), "rayrs_lab_radiance_tuning")

    def lab_probe_project_ms(self, n: int, samples: int, sample_chunk: int = 0, repeats: int = 10) -> float:
        """rayrs_amd/csrc/rayrs_lab.h rayrs_lab_probe_project_ms: for scripts/ubench only; ms of one projection of n probes."""
        ms = C.c_float()
        _ffi.check(self._L.rayrs_lab_probe_project_ms(self._h, int(n), int(samples), int(sample_chunk), int(repeats), C.addressof(ms)),
                   "rayrs_lab_probe_project_ms")
        return ms.value

    def close(self):
        if self._h is not None:
            self._L.rayrs_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def frame_sample_chunk(width: int, height: int, spp: int, requested: int = 4) -> int:
    """The sample chunk bench.py, the CLI and the full-size tests render a frame with: decided
    from the whole frame (never from the number of GPUs sharing it), so every rank count sums a
    pixel's samples in the same order.  0 = one sequential sum (the reference's order)."""
    return int(_ffi.lib().rayrs_frame_sample_chunk(int(width), int(height), int(spp), int(requested)))


def make_params(spp, max_bounces=50, seed=0x5EED, sample_chunk=0, tile_rank=0, tile_ranks=1, out_f64=False,
                count_work=False, exact_traversal=True, fast_traversal=None) -> _ffi.RenderParams:
    """exact_traversal=True (the default): the reference's visit set by construction; False, or fast_traversal=True:
    the fast walk (include/rayrs_hip.h rayrs_render_params.fast_traversal)."""
    p = _ffi.RenderParams()
    p.spp, p.max_bounces, p.seed = int(spp), int(max_bounces), int(seed)
    p.sample_chunk, p.tile_rank, p.tile_ranks = int(sample_chunk), int(tile_rank), int(tile_ranks)
    p.out_format = 1 if out_f64 else 0
    p.count_work = 1 if count_work else 0
    fast = (not exact_traversal) if fast_traversal is None else bool(fast_traversal)
    p.fast_traversal = 1 if fast else 0
    return p


def render(scene: Scene, camera: Camera, spp: int, max_bounces: int = 50, seed: int = 0x5EED, sample_chunk: int = 0,
           tile_rank: int = 0, tile_ranks: int = 1, out_f64: bool = False, count_work: bool = False, out=None,
           exact_traversal: bool = True, fast_traversal=None):
    """The block loop of rayrs/src/main.rs:57-101 on the GPU.

    Returns (image, stats): image is (y_pixels, x_pixels, 3), f32 (what
    Image::pixels_f32 yields, image.rs:224) or f64 with out_f64; stats holds the
    ray/path counters, the NaN/negative pixel counts of main.rs:81-87 and the
    HIP-event time of the kernel.
    """
    L = scene._L
    H, W = camera.y_pixels(), camera.x_pixels()
    dt = np.float64 if out_f64 else np.float32
    if out is None:
        out = np.zeros((H, W, 3), dtype=dt)
    assert out.shape == (H, W, 3) and out.dtype == dt and out.flags.c_contiguous
    p = make_params(spp, max_bounces, seed, sample_chunk, tile_rank, tile_ranks, out_f64, count_work, exact_traversal,
                    fast_traversal)
    st = _ffi.RenderStats()
    _ffi.check(L.rayrs_render(scene._h, C.byref(camera.desc), C.byref(p), out.ctypes.data, C.byref(st)),
               "rayrs_render")
    return out, st.as_dict()


def render_multi(scene_list, camera: Camera, spp: int, max_bounces: int = 50, seed: int = 0x5EED,
                 sample_chunk: int = 0, out_f64: bool = False):
    """The block loop of rayrs/src/main.rs:57-101 over several GPUs inside the library: scene i
    renders the tiles t % n == i on its own host thread and stream, one RCCL reduce of the
    framebuffers assembles the frame on the first scene's device.  Returns (image, summed stats)."""
    L = scene_list[0]._L
    H, W = camera.y_pixels(), camera.x_pixels()
    out = np.zeros((H, W, 3), dtype=np.float64 if out_f64 else np.float32)
    p = make_params(spp, max_bounces, seed, sample_chunk, 0, 1, out_f64, False)
    st = _ffi.RenderStats()
    handles = (C.c_void_p * len(scene_list))(*[s._h for s in scene_list])
    _ffi.check(L.rayrs_render_multi(handles, len(scene_list), C.byref(camera.desc), C.byref(p), out.ctypes.data,
                                    C.byref(st)), "rayrs_render_multi")
    return out, st.as_dict()


def render_launch(scene: Scene, camera: Camera, params: _ffi.RenderParams, out_device_ptr: int, stream: int = 0):
    """Enqueue a render writing a DEVICE buffer (e.g. torch tensor .data_ptr())."""
    _ffi.check(scene._L.rayrs_render_launch(scene._h, C.byref(camera.desc), C.byref(params),
                                            C.c_void_p(out_device_ptr), C.c_void_p(stream)), "rayrs_render_launch")


def render_finish(scene: Scene) -> dict:
    st = _ffi.RenderStats()
    _ffi.check(scene._L.rayrs_render_finish(scene._h, C.byref(st)), "rayrs_render_finish")
    return st.as_dict()


# ---- first-hit features and the feature-guided filter (include/rayrs_hip.h FEATURES, DENOISER)

# Starting points for the filter's sigmas, chosen by eye on the docs/renders scenes at 16 to 64 samples; nothing more.  A
# sigma is the distance at which a tap's weight has fallen to 1/e: of unit normals, of albedo, of depth as a fraction of
# the scene's root-box diagonal, of colour at level 0 (each level halves the colour sigma: kc_k = kc * 4^k).
SIGMA_NORMAL = 0.25
SIGMA_ALBEDO = 0.1
SIGMA_DEPTH_FRACTION = 0.02
SIGMA_COLOR = 0.6
# The guided filter's luminance sigma, in estimated standard deviations of the pixel (kv = 1 / 16): SVGF's value (Schied et
# al. 2017), a starting point and not tuned here.
SIGMA_LUMINANCE = 4.0


def _k(sigma) -> float:
    """1 / sigma^2; None or inf: the term is switched off."""
    if sigma is None or sigma == float("inf"):
        return 0.0
    sigma = float(sigma)
    return 1.0 / (sigma * sigma)


def scene_sigma_depth(scene: "Scene") -> float:
    """The default depth sigma: SIGMA_DEPTH_FRACTION of the scene's root-box diagonal."""
    b = scene.info()["root_box"]
    dx, dy, dz = b[1] - b[0], b[3] - b[2], b[5] - b[4]
    diag = float(np.sqrt(dx * dx + dy * dy + dz * dz))
    return SIGMA_DEPTH_FRACTION * diag if np.isfinite(diag) and diag > 0.0 else None


def _feature_planes(H, W):
    return {"normal": np.zeros((H, W, 3)), "albedo": np.zeros((H, W, 3)), "depth": np.zeros((H, W)),
            "coverage": np.zeros((H, W)), "object": np.zeros((H, W), dtype=np.uint32)}


def render_features(scene: Scene, camera: Camera, samples: int = 16, seed: int = 0x5EED, tile_rank: int = 0,
                    tile_ranks: int = 1, fast_traversal: bool = False) -> dict:
    """First-hit feature buffers of the view, averaged over `samples` samples per pixel: a dict of "normal" and "albedo"
    (H, W, 3) f64, "depth" and "coverage" (H, W) f64 and "object" (H, W) uint32 -- the object sample 0 hit, in insertion
    order, 0xFFFFFFFF for none.  Pixels outside the tile share read 0 and 0xFFFFFFFF."""
    out = _feature_planes(camera.y_pixels(), camera.x_pixels())
    _ffi.check(scene._L.rayrs_render_features(scene._h, C.byref(camera.desc), int(samples), int(seed), int(tile_rank),
                                              int(tile_ranks), int(fast_traversal), out["normal"].ctypes.data,
                                              out["albedo"].ctypes.data, out["depth"].ctypes.data, out["coverage"].ctypes.data,
                                              out["object"].ctypes.data), "rayrs_render_features")
    return out


def render_ao(scene: Scene, camera: Camera, samples: int = 16, t_max=None, bias: float = 0.0, seed: int = 0x5EED,
              ao_seed: int = 0xA0, fast_traversal: bool = False, counts: bool = False):
    """The ambient-occlusion plane of the view (include/rayrs_hip.h AMBIENT OCCLUSION PLANE): (H, W) f64 visibility at the
    first hit of every pixel's sample 0, exactly 1.0 where the primary ray misses; with counts also the (H, W) uint32 counts."""
    H, W = camera.y_pixels(), camera.x_pixels()
    vis, cnt = np.zeros((H, W)), np.zeros((H, W), dtype=np.uint32)
    _ffi.check(scene._L.rayrs_render_ao(scene._h, C.byref(camera.desc), int(seed), int(ao_seed), int(samples),
                                        float("inf") if t_max is None else float(t_max), float(bias), int(bool(fast_traversal)),
                                        cnt.ctypes.data, vis.ctypes.data), "rayrs_render_ao")
    return (vis, cnt) if counts else vis


# The sky in a light list: the number Scene.intersect returns as `object` for a miss (include/rayrs_hip.h SKY SAMPLING).
SKY = 0xFFFFFFFF


def _light_list(lights):
    """A light list as the contiguous uint32 host array the library reads."""
    lights = np.ascontiguousarray(lights, dtype=np.int64).reshape(-1)
    if len(lights) and (lights.min() < 0 or lights.max() > 0xFFFFFFFF):
        raise ValueError("a light is an object index, 0 .. 2^32 - 1")
    return lights.astype(np.uint32)


def emitters(objects) -> List[int]:
    """The indices, in the scene's numbering (Scene.intersect's `object`: insertion order, a mesh one index per triangle), of
    the emissive sphere and plane objects of an object list: what radiance(), irradiance() and render_lit() take as lights."""
    out, index = [], 0
    for o in flatten_objects(objects):
        if o.kind == "mesh":
            index += int(o.idx.shape[0])
            continue
        if o.kind in ("sphere", "plane") and o.emission.emissive:
            out.append(index)
        index += 1
    return out


def mesh_emitters(objects) -> List[int]:
    """The indices, in the scene's numbering, of the emissive triangles of an object list (a mesh: one index per triangle): what
    Scene.mesh_lights() takes."""
    out, index = [], 0
    for o in flatten_objects(objects):
        if o.kind == "mesh":
            n = int(o.idx.shape[0])
            if o.emission.emissive:
                out.extend(range(index, index + n))
            index += n
            continue
        if o.kind == "triangle" and o.emission.emissive:
            out.append(index)
        index += 1
    return out


# ---- SH probes on the host (include/rayrs_hip.h SH PROBES): no device is needed

def probe_directions(n: int, samples: int, seed: int = 0x5EED, index_base: int = 0):
    """The direction of every sample of the probes index_base .. index_base + n - 1 of a Scene.probes call: (n, samples, 3) f64."""
    n, samples = int(n), int(samples)
    if n < 0 or samples < 0:
        raise ValueError("n and samples must not be negative")
    out = np.zeros((n, samples, 3))
    buf = out if out.size else np.zeros(3)
    _ffi.check(_ffi.lib().rayrs_probe_directions(int(seed), int(index_base), n, samples, buf.ctypes.data), "rayrs_probe_directions")
    return out


def sh_basis(directions):
    """Y_0 .. Y_8 of every direction (m, 3), used as given: (m, 9) f64."""
    d = np.ascontiguousarray(directions, dtype=np.float64)
    if d.ndim != 2 or d.shape[1] != 3:
        raise ValueError("directions must be (m, 3)")
    out = np.zeros((max(len(d), 1), 9))
    _ffi.check(_ffi.lib().rayrs_sh_basis(d.ctypes.data if len(d) else out.ctypes.data, len(d), out.ctypes.data), "rayrs_sh_basis")
    return out[:len(d)]


_SH_K = (0.28209479177387814, 0.4886025119029199, 1.0925484305920792, 0.31539156525252005, 0.5462742152960396)
_SH_BAND = (1.0, 2.0 / 3.0, 2.0 / 3.0, 2.0 / 3.0, 0.25, 0.25, 0.25, 0.25, 0.25)   # clamped cosine over pi: 1, 2/3, 1/4 on l = 0, 1, 2


def _sh_eval(coeffs, directions, band):
    """sum_k band_k c_k Y_k(d): plain array arithmetic on numpy arrays or torch tensors, coeffs (..., 9, 3) and directions (..., 3)
    broadcast over their leading axes -> (..., 3)."""
    k0, k1, k2, k3, k4 = _SH_K
    x, y, z = directions[..., 0], directions[..., 1], directions[..., 2]
    Y = (k0 + 0.0 * x, k1 * y, k1 * z, k1 * x, k2 * x * y, k2 * y * z, k3 * (3.0 * z * z - 1.0), k2 * x * z, k4 * (x * x - y * y))
    out = None
    for k in range(9):
        term = (band[k] * Y[k])[..., None] * coeffs[..., k, :]
        out = term if out is None else out + term
    return out


def sh_radiance(coeffs, directions):
    """The radiance the coefficients stand for in every direction, sum_k c_k Y_k(d): coeffs (..., 9, 3), directions (..., 3)
    of unit length, broadcast over the leading axes -> (..., 3).  numpy in, numpy out; torch in, torch out."""
    return _sh_eval(coeffs, directions, (1.0,) * 9)


def sh_irradiance(coeffs, normals):
    """The clamped-cosine convolution of the coefficients around every normal, divided by pi: Scene.irradiance's unit (a
    Lambertian texel of albedo rho radiates rho times the value).  The band factors are 1, 2/3 and 1/4 on l = 0, 1, 2.  Shapes and
    array kinds as sh_radiance()."""
    return _sh_eval(coeffs, normals, _SH_BAND)


def probe_grid(scene: Scene, shape):
    """(nx * ny * nz, 3) f64 points at the cell centres of a grid of `shape` = (nx, ny, nz) cells over the scene's root box, x
    fastest: probe positions for Scene.probes.  A scene whose root box is not finite (an unbounded plane) has no grid."""
    nx, ny, nz = (int(v) for v in shape)
    if min(nx, ny, nz) < 1:
        raise ValueError("shape must be three positive cell counts")
    b = np.array(scene.info()["root_box"], dtype=np.float64)
    if not np.isfinite(b).all():
        raise ValueError("the scene's root box is not finite: give the probe positions yourself")
    axes = [b[2 * a] + (np.arange(m) + 0.5) * ((b[2 * a + 1] - b[2 * a]) / m) for a, m in enumerate((nx, ny, nz))]
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return np.ascontiguousarray(np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1))


class MeshLights:
    """A mesh-light group (include/rayrs_hip.h MESH LIGHTS): listed triangles of one scene that together are one more light of
    direct lighting.  The table lives on the host; its device copy is made by the first call that launches."""

    def __init__(self, scene: Scene, tris, tree: bool = False):
        tris = _light_list(tris)
        self._L, self._h, self._scene = scene._L, None, scene   # (the scene outlives the handle)
        self.tree = bool(tree)   # LIGHT TREE: the triangle is chosen by the tree's descent from the shading point
        h = C.c_void_p()
        name = "rayrs_mesh_lights_create_tree" if self.tree else "rayrs_mesh_lights_create"
        _ffi.check(getattr(self._L, name)(scene._h, tris.ctypes.data if len(tris) else None, len(tris), C.byref(h)), name)
        self._h, self._n = h, len(tris)

    def _handle(self):
        if self._h is None:
            raise ValueError("the mesh-light group is closed")
        return self._h

    def __len__(self):
        return self._n

    def areas(self):
        """A_j of every entry, in list order: (N,) f64."""
        out, total = np.zeros(max(self._n, 1)), C.c_double()
        _ffi.check(self._L.rayrs_mesh_lights_table(self._handle(), out.ctypes.data, C.addressof(total)), "rayrs_mesh_lights_table")
        return out[:self._n]

    @property
    def total(self) -> float:
        """T, the group's area."""
        total = C.c_double()
        _ffi.check(self._L.rayrs_mesh_lights_table(self._handle(), None, C.addressof(total)), "rayrs_mesh_lights_table")
        return total.value

    def _need_tree(self):
        if not self.tree:
            raise ValueError("the mesh-light group has no light tree (Scene.mesh_lights(tris, tree=True))")

    def powers(self):
        """LIGHT TREE: w_j of every entry, in list order: (N,) f64."""
        self._need_tree()
        out = np.zeros(max(self._n, 1))
        _ffi.check(self._L.rayrs_mesh_lights_tree_entries(self._handle(), out.ctypes.data, None, None), "rayrs_mesh_lights_tree_entries")
        return out[:self._n]

    def paths(self):
        """LIGHT TREE: (path word (N,) uint32, depth (N,) uint32) of every entry's leaf; bit k of the word: right at depth k."""
        self._need_tree()
        path, depth = np.zeros(max(self._n, 1), dtype=np.uint32), np.zeros(max(self._n, 1), dtype=np.uint32)
        _ffi.check(self._L.rayrs_mesh_lights_tree_entries(self._handle(), None, path.ctypes.data, depth.ctypes.data),
                   "rayrs_mesh_lights_tree_entries")
        return path[:self._n], depth[:self._n]

    def nodes(self):
        """LIGHT TREE: the 2N - 1 nodes in preorder: (m, r2, W (2N-1, 5) f64, right (2N-1,) uint32, entry (2N-1,) uint32), with
        0xFFFFFFFF for a leaf's right child and an interior node's entry."""
        self._need_tree()
        k = max(2 * self._n - 1, 0)
        mrw, right, entry = np.zeros((max(k, 1), 5)), np.zeros(max(k, 1), dtype=np.uint32), np.zeros(max(k, 1), dtype=np.uint32)
        _ffi.check(self._L.rayrs_mesh_lights_tree_nodes(self._handle(), mrw.ctypes.data, right.ctypes.data, entry.ctypes.data),
                   "rayrs_mesh_lights_tree_nodes")
        return mrw[:k], right[:k], entry[:k]

    def probability(self, positions, j):
        """LIGHT TREE: tree_probability(position, j) of every row: (n,) f64."""
        self._need_tree()
        p = np.ascontiguousarray(positions, dtype=np.float64)
        j = _light_list(j)
        if p.ndim != 2 or p.shape[1] != 3 or len(j) != len(p):
            raise ValueError("positions must be (n, 3), j (n,)")
        out = np.zeros(max(len(p), 1))
        _ffi.check(self._L.rayrs_mesh_lights_tree_probability(self._handle(), (p if len(p) else np.zeros((1, 3))).ctypes.data,
                                                              (j if len(p) else np.zeros(1, dtype=np.uint32)).ctypes.data, len(p),
                                                              out.ctypes.data), "rayrs_mesh_lights_tree_probability")
        return out[:len(p)]

    def sample(self, u, positions=None):
        """mesh_sample(u1, u2) of every row of u (n, 2): (j (n,) uint32, q (n, 3) f64), points uniform by area over the group.
        LIGHT TREE: tree_sample(position, u1, u2) of every row, with positions (n, 3): (j, q, p_sel (n,) f64)."""
        u = np.ascontiguousarray(u, dtype=np.float64)
        if u.ndim != 2 or u.shape[1] != 2:
            raise ValueError("u must be (n, 2)")
        m = max(len(u), 1)
        j, q = np.zeros(m, dtype=np.uint32), np.zeros((m, 3))
        if self.tree and positions is not None:
            p = np.ascontiguousarray(positions, dtype=np.float64)
            if p.shape != (len(u), 3):
                raise ValueError("positions must be (n, 3)")
            p_sel = np.zeros(m)
            _ffi.check(self._L.rayrs_mesh_lights_tree_sample(self._handle(), (p if len(u) else q).ctypes.data,
                                                             (u if len(u) else q).ctypes.data, len(u), j.ctypes.data, q.ctypes.data,
                                                             p_sel.ctypes.data), "rayrs_mesh_lights_tree_sample")
            return j[:len(u)], q[:len(u)], p_sel[:len(u)]
        if positions is not None:
            raise ValueError("positions=... is a light tree's (Scene.mesh_lights(tris, tree=True))")
        _ffi.check(self._L.rayrs_mesh_lights_sample(self._handle(), u.ctypes.data if len(u) else q.ctypes.data, len(u), j.ctypes.data,
                                                    q.ctypes.data), "rayrs_mesh_lights_sample")
        return j[:len(u)], q[:len(u)]

    def density(self, positions, j, q):
        """p_tri of every (position, j, q): the solid-angle density at the position of sample()'s points at q, (n,) f64 (a tree
        group: LIGHT TREE's p_tri, with the tree's probability of j at the position)."""
        p = np.ascontiguousarray(positions, dtype=np.float64)
        q = np.ascontiguousarray(q, dtype=np.float64)
        j = _light_list(j)
        if p.ndim != 2 or p.shape[1] != 3 or q.shape != p.shape or len(j) != len(p):
            raise ValueError("positions and q must be (n, 3), j (n,)")
        m = max(len(p), 1)
        out = np.zeros(m)
        pad = np.zeros((1, 3))
        _ffi.check(self._L.rayrs_mesh_lights_density(self._handle(), (p if len(p) else pad).ctypes.data,
                                                     (j if len(p) else np.zeros(1, dtype=np.uint32)).ctypes.data,
                                                     (q if len(p) else pad).ctypes.data, len(p), out.ctypes.data),
                   "rayrs_mesh_lights_density")
        return out[:len(p)]

    def close(self):
        if self._h is not None:
            # (a scene that is already closed took the device with it, and the library's destructor would read the freed scene:
            # garbage collection at interpreter exit finalizes a scene and its dependents in any order)
            if self._scene._h is not None:
                self._L.rayrs_mesh_lights_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def render_lit(scene: Scene, camera: Camera, samples: int, lights, max_bounces: int = 50, seed: int = 0x5EED, sample_chunk: int = 0,
               fast_traversal: bool = False, queries: bool = False, mesh: Optional[MeshLights] = None, direct: bool = False):
    """The view's radiance with light sampling (include/rayrs_hip.h LIGHT SAMPLING, the image form): (H, W, 3) f64, the mean of
    `samples` paths per pixel whose diffuse surfaces sample `lights` half of the time; with queries also the (H, W) uint32
    closest-hit queries per pixel.  With an empty list the frame is render(..., out_f64=True)'s, bit for bit.  direct=True:
    DIRECT LIGHTING's image form instead, a shadow ray per diffuse bounce beside the surface's own direction; with SKY in the
    list, SKY SAMPLING's: the environment map is one more of the lights; with mesh (a Scene.mesh_lights() group), MESH LIGHTS':
    its triangles are one more of them."""
    if direct and lights is None:
        raise ValueError("direct=True needs a light list (lights=[...])")
    if mesh is not None and not direct:
        raise ValueError("mesh=... needs direct=True (a mesh-light group is a light of direct lighting)")
    H, W = camera.y_pixels(), camera.x_pixels()
    lights = _light_list(lights)
    sky = bool(direct) and bool((lights == SKY).any())
    if sky:
        lights = lights[lights != SKY]
    out, cnt = np.zeros((H, W, 3)), np.zeros((H, W), dtype=np.uint32)
    name = "rayrs_render_mesh" if mesh is not None else "rayrs_render_sky" if sky else "rayrs_render_direct" if direct else "rayrs_render_lit"
    extra = () if mesh is None else (mesh._handle(), int(sky))
    _ffi.check(getattr(scene._L, name)(scene._h, C.byref(camera.desc), int(seed), int(samples), int(max_bounces), int(sample_chunk),
                                       int(bool(fast_traversal)), lights.ctypes.data if len(lights) else None, len(lights), *extra,
                                       out.ctypes.data, cnt.ctypes.data), name)
    return (out, cnt) if queries else out


def _filter_inputs(color, planes, what, variance=False):
    """What denoise() and denoise_guided() are given, checked: color as a contiguous f64 (H, W, 3) frame, and each of
    `planes` -- (array or None, its shape after (H, W)) -- likewise, None staying None.  `what` names a plane that has
    another shape in the ValueError; with `variance` the first plane is the variance, which may not be None."""
    color = np.ascontiguousarray(color, dtype=np.float64)
    if color.ndim != 3 or color.shape[2] != 3:
        raise ValueError("color must be (H, W, 3)")
    if variance and planes[0][0] is None:
        raise ValueError("variance must be (H, W)")
    checked = []
    for a, tail in planes:
        if a is not None:
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.shape != color.shape[:2] + tail:
                raise ValueError(f"{what} must be {color.shape[:2] + tail}")
        checked.append(a)
    return color, checked


def _ptr(a):
    return None if a is None else a.ctypes.data


def denoise(color, normal=None, albedo=None, depth=None, levels: int = 5, sigma_normal=SIGMA_NORMAL,
            sigma_albedo=SIGMA_ALBEDO, sigma_depth=None, sigma_color=SIGMA_COLOR, device: int = 0):
    """The edge-avoiding a-trous filter of include/rayrs_hip.h (DENOISER) on any (H, W, 3) frame, on the GPU; returns
    the filtered f64 frame.  A feature plane that is None contributes no term; a sigma that is None or inf switches its
    term off (sigma_depth has no default here: depth has no scale without a scene)."""
    color, (normal, albedo, depth) = _filter_inputs(color, [(normal, (3,)), (albedo, (3,)), (depth, ())], "feature plane")
    H, W = color.shape[:2]
    out = np.zeros((H, W, 3))
    _ffi.check(_ffi.lib().rayrs_image_denoise(int(device), W, H, color.ctypes.data, _ptr(normal), _ptr(albedo), _ptr(depth),
                                              int(levels), _k(sigma_normal), _k(sigma_albedo), _k(sigma_depth),
                                              _k(sigma_color), out.ctypes.data), "rayrs_image_denoise")
    return out


def denoise_guided(color, variance, normal=None, albedo=None, depth=None, levels: int = 5, sigma_normal=SIGMA_NORMAL,
                   sigma_albedo=SIGMA_ALBEDO, sigma_depth=None, sigma_luminance=SIGMA_LUMINANCE, device: int = 0,
                   return_variance: bool = False):
    """The variance-guided a-trous filter of include/rayrs_hip.h (GUIDED FILTER) on any (H, W, 3) frame with the (H, W)
    variance of its channel sums, on the GPU; returns the filtered f64 frame, or (frame, variance after the last level) with
    return_variance.  Planes and sigmas as denoise(); sigma_luminance is in standard deviations of the pixel."""
    color, (variance, normal, albedo, depth) = _filter_inputs(
        color, [(variance, ()), (normal, (3,)), (albedo, (3,)), (depth, ())], "plane", variance=True)
    H, W = color.shape[:2]
    out = np.zeros((H, W, 3))
    out_var = np.zeros((H, W)) if return_variance else None
    _ffi.check(_ffi.lib().rayrs_image_denoise_guided(int(device), W, H, color.ctypes.data, variance.ctypes.data, _ptr(normal),
                                                     _ptr(albedo), _ptr(depth), int(levels), _k(sigma_normal), _k(sigma_albedo),
                                                     _k(sigma_depth), _k(sigma_luminance), out.ctypes.data, _ptr(out_var)),
               "rayrs_image_denoise_guided")
    return (out, out_var) if return_variance else out


class Film:
    """A progressive film (include/rayrs_hip.h rayrs_film_*): samples are added to it pass by pass, and after passes
    that add up to N samples image() is, bit for bit, render(scene, camera, N, sample_chunk=sample_chunk) with the same
    seed, bounces, tile share and walk.  The scene must outlive the film.

    With lights=[...] and direct=True the film is direct-lit (DIRECT-LIT FILMS): its passes take a shadow sample per diffuse
    bounce towards the list's lamps, and towards the sky too if SKY is in the list, and image() is
    render_lit(scene, camera, N, lights, direct=True, sample_chunk=sample_chunk), bit for bit.  The list is fixed for the
    film's life (film.lights); everything else a film does works on such a film unchanged.

    With mesh=group as well (MESH-LIT FILMS AND BAKES; a Scene.mesh_lights() group, lights may be empty) the group is one more
    of those lights and image() is render_lit(..., direct=True, mesh=group), bit for bit.  The film keeps a reference to the
    group (film.mesh), which must stay open while the film lives."""

    def __init__(self, scene: Scene, camera: Camera, sample_chunk: int = 4, max_bounces: int = 50, seed: int = 0x5EED,
                 tile_rank: int = 0, tile_ranks: int = 1, fast_traversal: bool = False, lights=None, direct: bool = False,
                 mesh: Optional["MeshLights"] = None):
        if mesh is not None and not direct:
            raise ValueError("mesh=... needs direct=True (a mesh-light group is a light of direct lighting)")
        if direct and lights is None:
            raise ValueError("direct=True needs a light list (lights=[...])")
        if lights is not None and not direct:
            raise ValueError("a film with a light list is direct-lit: pass direct=True (the one-sample mix has no film)")
        self._L, self._h = scene._L, None
        self.scene, self.camera = scene, camera
        self.lights = None if lights is None else [int(v) for v in _light_list(lights)]
        self.mesh = mesh
        p = _ffi.FilmParams()
        p.sample_chunk, p.max_bounces, p.seed = int(sample_chunk), int(max_bounces), int(seed)
        p.tile_rank, p.tile_ranks, p.fast_traversal = int(tile_rank), int(tile_ranks), 1 if fast_traversal else 0
        self.sample_chunk = int(sample_chunk) or 4
        self.tile_rank, self.tile_ranks = int(tile_rank), int(tile_ranks) or 1
        h = C.c_void_p()
        if lights is None:
            _ffi.check(self._L.rayrs_film_create(scene._h, C.byref(camera.desc), C.byref(p), C.byref(h)), "rayrs_film_create")
        else:  # (the rule render_lit chooses its entry point by: SKY in the list is the sky, the rest the lamps)
            lamps = _light_list(lights)
            sky = bool((lamps == SKY).any())
            name = "rayrs_film_create_mesh" if mesh is not None else "rayrs_film_create_sky" if sky else "rayrs_film_create_direct"
            lamps = lamps[lamps != SKY]
            extra = () if mesh is None else (mesh._handle(), int(sky))  # (the group and the sky as arguments of their own)
            _ffi.check(getattr(self._L, name)(scene._h, C.byref(camera.desc), C.byref(p), lamps.ctypes.data if len(lamps) else None,
                                              len(lamps), *extra, C.byref(h)), name)
        self._h = h

    def render(self, n: int) -> dict:
        """Adds n samples to every pixel; the pass's counters and times (as render()'s stats).  n that is not a
        multiple of sample_chunk closes the film: no further pass is accepted."""
        st = _ffi.RenderStats()
        _ffi.check(self._L.rayrs_film_render(self._h, int(n), C.byref(st)), "rayrs_film_render")
        return st.as_dict()

    def render_adaptive(self, n: int, tau: float, max_tile_samples: int = 0):
        """Adds n samples (a multiple of sample_chunk) to the 8x8 tiles of the share that hold a pixel unconverged at
        tau and at most max_tile_samples - n samples (0: no cap).  Returns (active_tiles, stats); no tile selected is
        (0, zeroed stats) and leaves the film as it is."""
        st, active = _ffi.RenderStats(), C.c_uint64(0)
        _ffi.check(self._L.rayrs_film_render_adaptive(self._h, int(n), float(tau), int(max_tile_samples), C.byref(active),
                                                      C.byref(st)), "rayrs_film_render_adaptive")
        return int(active.value), st.as_dict()

    def tile_samples(self):
        """Samples per 8x8 tile of the frame, (tiles_y, tiles_x) uint32; 0 outside the film's share."""
        ty, tx = (self.camera.y_pixels() + 7) // 8, (self.camera.x_pixels() + 7) // 8
        out = np.zeros((ty, tx), dtype=np.uint32)
        if int(self._L.rayrs_film_tile_samples(self._h, out.ctypes.data, out.size)) != out.size:
            raise RuntimeError("rayrs_film_tile_samples: the film has another number of tiles than its camera")
        return out

    def sample_map(self):
        """Samples per pixel, (y_pixels, x_pixels) uint32: tile_samples() spread over the pixels."""
        per_tile = self.tile_samples()
        return np.repeat(np.repeat(per_tile, 8, axis=0), 8, axis=1)[:self.camera.y_pixels(), :self.camera.x_pixels()].copy()

    def image(self, out_f64: bool = False):
        """The frame as it stands: (y_pixels, x_pixels, 3), f32 or f64 (a tile's sum over its own sample count)."""
        out = np.zeros((self.camera.y_pixels(), self.camera.x_pixels(), 3), dtype=np.float64 if out_f64 else np.float32)
        _ffi.check(self._L.rayrs_film_read(self._h, 1 if out_f64 else 0, out.ctypes.data), "rayrs_film_read")
        return out

    def features(self, samples: int = 16) -> dict:
        """render_features() with the film's camera, seed, tile share and walk; independent of the samples the film holds,
        and without effect on them."""
        out = _feature_planes(self.camera.y_pixels(), self.camera.x_pixels())
        _ffi.check(self._L.rayrs_film_features(self._h, int(samples), out["normal"].ctypes.data, out["albedo"].ctypes.data,
                                               out["depth"].ctypes.data, out["coverage"].ctypes.data, out["object"].ctypes.data),
                   "rayrs_film_features")
        return out

    def _filter_ks(self, sigma_normal, sigma_albedo, sigma_depth, sigma_last):
        """The four k of a filter call from its sigmas; sigma_depth given as a string: the scene's default."""
        if isinstance(sigma_depth, str):
            sigma_depth = scene_sigma_depth(self.scene)
        return _k(sigma_normal), _k(sigma_albedo), _k(sigma_depth), _k(sigma_last)

    def denoised(self, levels: int = 5, feature_samples: int = 16, sigma_normal=SIGMA_NORMAL, sigma_albedo=SIGMA_ALBEDO,
                 sigma_depth="scene", sigma_color=SIGMA_COLOR, out_f64: bool = False):
        """image(out_f64=True) filtered on the device with the normal, albedo and depth of `feature_samples` samples
        (include/rayrs_hip.h DENOISER); f32, or f64 with out_f64.  The film itself is unchanged.  The default sigmas
        are starting points chosen by eye (SIGMA_* above), sigma_depth a fraction of the scene's root-box diagonal; None or
        inf switches a term off."""
        out = np.zeros((self.camera.y_pixels(), self.camera.x_pixels(), 3), dtype=np.float64 if out_f64 else np.float32)
        _ffi.check(self._L.rayrs_film_denoise(self._h, int(feature_samples), int(levels),
                                              *self._filter_ks(sigma_normal, sigma_albedo, sigma_depth, sigma_color),
                                              1 if out_f64 else 0, out.ctypes.data), "rayrs_film_denoise")
        return out

    def noise(self):
        """The film's noise estimate per pixel, (y_pixels, x_pixels) f64 (include/rayrs_hip.h NOISE PLANE): the batch-means
        variance of the channel sum of the frame image() returns; +inf where a tile holds fewer than two full chunks, 0
        outside the film's share."""
        out = np.zeros((self.camera.y_pixels(), self.camera.x_pixels()))
        _ffi.check(self._L.rayrs_film_noise(self._h, out.ctypes.data), "rayrs_film_noise")
        return out

    def denoised_guided(self, levels: int = 5, feature_samples: int = 16, sigma_normal=SIGMA_NORMAL, sigma_albedo=SIGMA_ALBEDO,
                        sigma_depth="scene", sigma_luminance=SIGMA_LUMINANCE, out_f64: bool = False,
                        return_variance: bool = False):
        """image(out_f64=True) filtered on the device with noise() and the normal, albedo and depth of `feature_samples`
        samples (include/rayrs_hip.h GUIDED FILTER): a tap's luminance difference is measured in the pixel's own estimated
        standard deviations, so tiles that stopped at different sample counts are each filtered by their own noise.  f32,
        or f64 with out_f64; with return_variance (frame, the variance left after the last level).  The film itself is
        unchanged.  Sigmas as denoised(); where noise() is +inf the result is denoised(sigma_color=None)."""
        H, W = self.camera.y_pixels(), self.camera.x_pixels()
        out = np.zeros((H, W, 3), dtype=np.float64 if out_f64 else np.float32)
        out_var = np.zeros((H, W)) if return_variance else None
        _ffi.check(self._L.rayrs_film_denoise_guided(self._h, int(feature_samples), int(levels),
                                                     *self._filter_ks(sigma_normal, sigma_albedo, sigma_depth, sigma_luminance),
                                                     1 if out_f64 else 0, out.ctypes.data, _ptr(out_var)),
                   "rayrs_film_denoise_guided")
        return (out, out_var) if return_variance else out

    def status(self, tau: float = 0.0) -> dict:
        """samples, full_chunks, rays, paths, nan_pixels, neg_pixels, closed, and for this tau the batch-means noise
        estimate's counts unconverged and nonfinite (include/rayrs_hip.h NOISE)."""
        st = _ffi.FilmStatus()
        _ffi.check(self._L.rayrs_film_status_get(self._h, float(tau), C.byref(st)), "rayrs_film_status_get")
        return st.as_dict()

    def pixels(self) -> int:
        """Pixels of the film's share (what status()["unconverged"] counts among)."""
        from . import tiles
        return int(tiles.tile_mask(self.camera.x_pixels(), self.camera.y_pixels(), self.tile_rank, self.tile_ranks).sum())

    def state(self) -> bytes:
        n = int(self._L.rayrs_film_state_bytes(self._h))
        buf = np.zeros(n, dtype=np.uint8)
        _ffi.check(self._L.rayrs_film_state_get(self._h, buf.ctypes.data, n), "rayrs_film_state_get")
        return buf.tobytes()

    def set_state(self, image: bytes):
        buf = np.frombuffer(image, dtype=np.uint8)
        _ffi.check(self._L.rayrs_film_state_set(self._h, buf.ctypes.data, len(buf)), "rayrs_film_state_set")

    def save(self, path):
        """The film's byte image in a file, nothing else."""
        with open(path, "wb") as f:
            f.write(self.state())

    def load(self, path):
        """Continue from a saved film: refused (RayrsError, the film unchanged) unless the image was made with this
        film's image size, sample_chunk, seed, max_bounces, tile share and walk."""
        with open(path, "rb") as f:
            self.set_state(f.read())

    def close(self):
        if self._h is not None:
            # (a scene that is already closed took the device with it, and the library's destructor would read the freed scene:
            # garbage collection at interpreter exit finalizes a scene and its dependents in any order)
            if self.scene._h is not None:
                self._L.rayrs_film_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def render_until(film, tau: float, max_unconverged_fraction: float = 0.0, pass_samples: int = 16, max_samples: int = 1024,
                 time_budget_s: Optional[float] = None, on_pass=None, adaptive: bool = False):
    """Adds passes of pass_samples samples (rounded up to a multiple of the film's sample_chunk) until at most
    max_unconverged_fraction of its pixels are unconverged at tau ("converged"), or the next
    pass would take the film beyond max_samples ("max_samples"), or time_budget_s seconds have passed ("time_budget").
    on_pass(film, status) is called after every pass.  Returns (status, reason); the status is film.status(tau) as it
    stands, with "pixels" added.
    adaptive: the passes are film.render_adaptive(step, tau, max_samples) -- only the tiles that still hold an unconverged
    pixel get samples, none beyond max_samples -- and "max_samples" is a pass that selects no tile while pixels are still
    unconverged; the status then also has "active_tiles" of the last pass, "tile_samples_min" and "tile_samples_max" over
    the share's tiles, and "pixel_samples", the samples summed over the share's pixels."""
    import time
    c = int(film.sample_chunk)
    step = -(-int(pass_samples) // c) * c
    if step <= 0:
        raise ValueError("pass_samples must be positive")
    pixels = int(film.pixels())
    t0 = time.monotonic()

    def done(st):
        return st["samples"] > 0 and st["unconverged"] <= max_unconverged_fraction * pixels

    st = film.status(tau)
    while True:
        if done(st):
            reason = "converged"
            break
        if st["closed"] or (max_samples < step if adaptive else st["samples"] + step > max_samples):
            reason = "max_samples"
            break
        if time_budget_s is not None and time.monotonic() - t0 >= time_budget_s:
            reason = "time_budget"
            break
        if adaptive:
            active, _ = film.render_adaptive(step, tau, max_samples)
            if active == 0:  # every tile that is still noisy has its max_samples
                reason = "max_samples"
                break
        else:
            film.render(step)
        st = film.status(tau)
        if adaptive:
            st = dict(st, active_tiles=active)
        if on_pass is not None:
            on_pass(film, st)
    st = dict(st)
    st["pixels"] = pixels
    if adaptive:
        from . import tiles
        cam = film.camera
        per_pixel = film.sample_map()[tiles.tile_mask(cam.x_pixels(), cam.y_pixels(), film.tile_rank, film.tile_ranks)]
        st["tile_samples_min"] = int(per_pixel.min()) if per_pixel.size else 0
        st["tile_samples_max"] = int(per_pixel.max()) if per_pixel.size else 0
        st["pixel_samples"] = int(per_pixel.astype(np.uint64).sum())
    return st, reason


# ---- the bake (include/rayrs_hip.h BAKE)

class Bake:
    """Progressive, adaptive radiance queries at fixed points (include/rayrs_hip.h BAKE): a device-resident accumulation
    buffer over the n rays or points (a, b) -- kind="irradiance": points and normals, kind="radiance": origins and directions,
    host arrays of shape (n, 3) -- to which samples are added pass by pass, to every point or only to the noisy ones.  After
    passes that leave point i at N_i samples, values()[i] is, bit for bit, scene.irradiance (scene.radiance) of that one point
    with samples=N_i, sample_chunk=sample_chunk, index_base=index_base + i and the same seed, bounces, bias, walk and lights.
    lights and direct as the queries take them: direct=True with a list is the direct-lit bake, SKY in the list the sky bake;
    a list without direct=True (the one-sample mix) has no bake.  mesh=group (with direct=True; lights may be empty): a
    Scene.mesh_lights() group as one more of those lights (MESH-LIT FILMS AND BAKES), the matching query then being the one
    with mesh=group; the bake keeps a reference to the group (bake.mesh), which must stay open while the bake lives.  The
    scene must outlive the bake."""

    def __init__(self, scene: Scene, a, b, kind: str = "irradiance", sample_chunk: int = 4, max_bounces: int = 50, seed: int = 0,
                 index_base: int = 0, bias: float = 0.0, fast_traversal: bool = False, lights=None, direct: bool = False,
                 mesh: Optional["MeshLights"] = None):
        if kind not in ("irradiance", "radiance"):
            raise ValueError('kind is "irradiance" or "radiance"')
        if mesh is not None and not direct:
            raise ValueError("mesh=... needs direct=True (a mesh-light group is a light of direct lighting)")
        if direct and lights is None:
            raise ValueError("direct=True needs a light list (lights=[...])")
        if lights is not None and not direct:
            raise ValueError("a bake with a light list is direct-lit: pass direct=True (the one-sample mix has no bake)")
        a, b = (np.ascontiguousarray(x, dtype=np.float64) for x in (a, b))
        if a.ndim != 2 or a.shape[1] != 3 or a.shape != b.shape:
            raise ValueError("a and b are arrays of shape (n, 3)")
        self._L, self._h = scene._L, None
        self.scene, self.kind, self.n = scene, kind, int(a.shape[0])
        self.sample_chunk = int(sample_chunk) or 4
        self.lights = None if lights is None else [int(v) for v in _light_list(lights)]
        self.mesh = mesh
        p = _ffi.BakeParams()
        p.kind, p.sample_chunk, p.max_bounces = 0 if kind == "irradiance" else 1, int(sample_chunk), int(max_bounces)
        p.fast_traversal, p.seed, p.index_base, p.bias = 1 if fast_traversal else 0, int(seed), int(index_base), float(bias)
        lamps = _light_list([] if lights is None else lights)
        p.sky = 1 if (lamps == SKY).any() else 0   # (the rule the queries choose their entry point by)
        lamps = lamps[lamps != SKY]
        if self.n == 0:
            a = b = np.zeros((1, 3))
        h = C.c_void_p()
        name = "rayrs_bake_create" if mesh is None else "rayrs_bake_create_mesh"
        extra = () if mesh is None else (mesh._handle(),)
        _ffi.check(getattr(self._L, name)(scene._h, a.ctypes.data, b.ctypes.data, self.n, C.byref(p),
                                          lamps.ctypes.data if len(lamps) else None, len(lamps), *extra, C.byref(h)), name)
        self._h = h

    def render(self, n: int) -> dict:
        """Adds n samples to every point from its own count; the pass's points, paths, rays, kernel_ms, total_ms and launches.
        n that is not a multiple of sample_chunk closes the bake: no further pass is accepted."""
        st = _ffi.BakePass()
        _ffi.check(self._L.rayrs_bake_render(self._h, int(n), C.byref(st)), "rayrs_bake_render")
        return st.as_dict()

    def render_adaptive(self, n: int, tau: float, max_point_samples: int = 0):
        """Adds n samples (a multiple of sample_chunk) to the points that are unconverged at tau and hold at most
        max_point_samples - n samples (0: no cap).  Returns (active_points, stats); no point selected is (0, zeroed stats) and
        leaves the bake as it is."""
        st, active = _ffi.BakePass(), C.c_uint64(0)
        _ffi.check(self._L.rayrs_bake_render_adaptive(self._h, int(n), float(tau), int(max_point_samples), C.byref(active),
                                                      C.byref(st)), "rayrs_bake_render_adaptive")
        return int(active.value), st.as_dict()

    def values(self, queries: bool = False):
        """The values as they stand, (n, 3) f64: a point's sum over its own sample count, +0 for a point without samples; with
        queries also the closest-hit queries its paths made, (n,) uint64."""
        m = max(self.n, 1)
        rad, cnt = np.zeros((m, 3)), np.zeros(m, dtype=np.uint64)
        _ffi.check(self._L.rayrs_bake_read(self._h, rad.ctypes.data, cnt.ctypes.data if queries else None), "rayrs_bake_read")
        return (rad[:self.n], cnt[:self.n]) if queries else rad[:self.n]

    def point_samples(self):
        """Samples per point, (n,) uint32."""
        out = np.zeros(max(self.n, 1), dtype=np.uint32)
        _ffi.check(self._L.rayrs_bake_point_samples(self._h, out.ctypes.data), "rayrs_bake_point_samples")
        return out[:self.n]

    def noise(self):
        """The noise estimate per point, (n,) f64 (include/rayrs_hip.h NOISE PLANE's formula): the batch-means variance of the
        channel sum of values(); +inf where a point holds fewer than two full chunks."""
        out = np.zeros(max(self.n, 1))
        _ffi.check(self._L.rayrs_bake_noise(self._h, out.ctypes.data), "rayrs_bake_noise")
        return out[:self.n]

    def status(self, tau: float = 0.0) -> dict:
        """samples (the largest per point), rays, paths, points, closed, and for this tau the noise estimate's counts
        unconverged and nonfinite (include/rayrs_hip.h NOISE)."""
        st = _ffi.BakeStatus()
        _ffi.check(self._L.rayrs_bake_status_get(self._h, float(tau), C.byref(st)), "rayrs_bake_status_get")
        return st.as_dict()

    def state(self) -> bytes:
        n = int(self._L.rayrs_bake_state_bytes(self._h))
        buf = np.zeros(n, dtype=np.uint8)
        _ffi.check(self._L.rayrs_bake_state_get(self._h, buf.ctypes.data, n), "rayrs_bake_state_get")
        return buf.tobytes()

    def set_state(self, image: bytes):
        buf = np.frombuffer(image, dtype=np.uint8)
        _ffi.check(self._L.rayrs_bake_state_set(self._h, buf.ctypes.data, len(buf)), "rayrs_bake_state_set")

    def save(self, path):
        """The bake's byte image in a file, nothing else (not the points, the scene or the lights)."""
        with open(path, "wb") as f:
            f.write(self.state())

    def load(self, path):
        """Continue from a saved bake: refused (RayrsError, the bake unchanged) unless the image was made with this bake's
        kind, strategy, sample_chunk, seed, index_base, bias, max_bounces, walk and number of points."""
        with open(path, "rb") as f:
            self.set_state(f.read())

    def close(self):
        if self._h is not None:
            # (a scene that is already closed took the device with it, and the library's destructor would read the freed scene:
            # garbage collection at interpreter exit finalizes a scene and its dependents in any order)
            if self.scene._h is not None:
                self._L.rayrs_bake_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def bake_until(bake, tau: float, pass_samples: int = 16, max_samples: int = 1024, adaptive: bool = True,
               time_budget: Optional[float] = None):
    """render_until for a bake: adds passes of pass_samples samples (rounded up to a multiple of the bake's sample_chunk) until
    no point is unconverged at tau ("converged"), or the next pass would take the bake beyond max_samples ("max_samples"), or
    time_budget seconds have passed ("time_budget").  adaptive: the passes are bake.render_adaptive(step, tau, max_samples) --
    only the points that are still unconverged get samples, none beyond max_samples -- and "max_samples" is a pass that selects
    no point while points are still unconverged.  Returns (status, reason); the status is bake.status(tau) as it stands with
    "point_samples" added, the samples summed over the points, and with adaptive "active_points" of the last pass."""
    import time
    c = int(bake.sample_chunk)
    step = -(-int(pass_samples) // c) * c
    if step <= 0:
        raise ValueError("pass_samples must be positive")
    t0 = time.monotonic()
    st = bake.status(tau)
    active = None
    while True:
        if (st["samples"] > 0 or st["points"] == 0) and st["unconverged"] == 0:
            reason = "converged"
            break
        if st["closed"] or (max_samples < step if adaptive else st["samples"] + step > max_samples):
            reason = "max_samples"
            break
        if time_budget is not None and time.monotonic() - t0 >= time_budget:
            reason = "time_budget"
            break
        if adaptive:
            active, _ = bake.render_adaptive(step, tau, max_samples)
            if active == 0:  # every point that is still noisy has its max_samples
                reason = "max_samples"
                break
        else:
            bake.render(step)
        st = bake.status(tau)
    st = dict(st)
    if adaptive and active is not None:
        st["active_points"] = active
    st["point_samples"] = int(bake.point_samples().astype(np.uint64).sum())
    return st, reason


# ---- lightmap atlases (include/rayrs_hip.h LIGHTMAP ATLAS)

LIGHTMAP_MAX_SIDE = 16384


def unwrap_triangles(m: int, cell: int = 8, gutter: int = 1):
    """A UV layout for m triangles that ignores the mesh's shape: (uvs (m, 3, 2) f64, width, height).  Triangles 2c and 2c + 1
    share square cell c -- `cell` texels a side, the cells row by row in a grid of ceil(sqrt(ceil(m / 2))) columns -- as the two
    right triangles on either side of its diagonal, each inset so that at least `gutter` texels lie between the texels of any two
    triangles (no texel one triangle covers has a texel of another within `gutter` steps, diagonal steps included).  The atlas
    is the grid's size times `cell`; the layout is a function of (m, cell, gutter) alone.  It is NOT a chart-preserving unwrap:
    neighbouring triangles of the mesh are not neighbours in the atlas, and every triangle gets the same texels whatever its
    size.  In cell coordinates (texels, L = cell - gutter, T = cell - 2 * gutter - 2) the even triangle is (0.25, 0.25),
    (T + 1.25, 0.25), (0.25, T + 1.25) and covers the texels i + j <= T; the odd one is (L - 0.25, L - 0.25), (T + 2 * gutter +
    1.75 - L, L - 0.25), (L - 0.25, T + 2 * gutter + 1.75 - L) and covers i + j >= T + 2 * gutter + 1 of 0 .. L - 1."""
    m, cell, gutter = int(m), int(cell), int(gutter)
    if m < 0 or gutter < 0 or cell < 2 * gutter + 2:
        raise ValueError("unwrap_triangles: m >= 0, gutter >= 0 and cell >= 2 * gutter + 2")
    cells = (m + 1) // 2
    cols = 1
    while cols * cols < cells:
        cols += 1
    rows = max(1, -(-cells // cols))
    width, height = cols * cell, rows * cell
    if width > LIGHTMAP_MAX_SIDE or height > LIGHTMAP_MAX_SIDE:
        raise ValueError(f"unwrap_triangles: a {width} x {height} atlas is above {LIGHTMAP_MAX_SIDE} a side")
    L, T = float(cell - gutter), float(cell - 2 * gutter - 2)
    lo = T + 2.0 * gutter + 1.75 - L
    corners = np.array([[(0.25, 0.25), (T + 1.25, 0.25), (0.25, T + 1.25)],
                        [(L - 0.25, L - 0.25), (lo, L - 0.25), (L - 0.25, lo)]])
    k = np.arange(m)
    c = k // 2
    origin = np.stack([(c % cols) * cell, (c // cols) * cell], axis=-1).astype(np.float64)   # (m, 2)
    uvs = (corners[k % 2] + origin[:, None, :]) / np.array([float(width), float(height)])
    return np.ascontiguousarray(uvs.reshape(m, 3, 2)), width, height


class Lightmap:
    """A lightmap atlas (include/rayrs_hip.h LIGHTMAP ATLAS): the triangles (verts (nv, 3) f32 or f64, idx (m, 3)) rasterised in
    UV space -- uvs per corner (m, 3, 2), or per vertex (nv, 2), expanded through idx -- into the texels of a width x height
    atlas on HIP device `device`.  n texels are owned; texels() gives their indices, world positions and normals (flip=True: the
    normals negated), which is what a Bake wants (bake()), and image() takes per-texel values back into an (H, W, C) picture with
    dilated chart borders.  Texel (x, y) has its centre at u = (x + 0.5) / width, v = (y + 0.5) / height, and row y of the image
    is v's: nothing is turned upside down.  The atlas is bound to no scene."""

    def __init__(self, verts, idx, uvs, width: int, height: int, flip: bool = False, device: int = 0):
        verts = np.ascontiguousarray(verts)
        if verts.dtype not in (np.float32, np.float64):
            verts = verts.astype(np.float64)
        idx = np.asarray(idx)
        if verts.ndim != 2 or verts.shape[1] != 3 or idx.ndim != 2 or idx.shape[1] != 3:
            raise ValueError("verts must be (nv, 3) and idx (m, 3)")
        if idx.dtype.kind not in "iu" or (idx.size and (int(idx.min()) < 0 or int(idx.max()) >= len(verts))):
            raise ValueError("idx must hold integers below the number of vertices")
        idx = np.ascontiguousarray(idx, dtype=np.uint32)
        uvs = np.ascontiguousarray(uvs, dtype=np.float64)
        if uvs.shape == (len(verts), 2) and uvs.shape != (len(idx), 3, 2):
            uvs = np.ascontiguousarray(uvs[idx.astype(np.int64)])
        if uvs.shape != (len(idx), 3, 2):
            raise ValueError("uvs must be (m, 3, 2) per corner or (nv, 2) per vertex")
        width, height = int(width), int(height)
        if not (1 <= width <= LIGHTMAP_MAX_SIDE and 1 <= height <= LIGHTMAP_MAX_SIDE):
            raise ValueError(f"width and height must be 1 .. {LIGHTMAP_MAX_SIDE}")
        self._L, self._h = _ffi.lib(), None
        self.width, self.height, self.flip, self.device, self.m = width, height, bool(flip), int(device), len(idx)
        dummy = np.zeros(6)
        h = C.c_void_p()
        _ffi.check(self._L.rayrs_lightmap_create(self.device, verts.ctypes.data if len(verts) else dummy.ctypes.data,
                                                 1 if verts.dtype == np.float32 else 0, len(verts),
                                                 idx.ctypes.data if len(idx) else dummy.ctypes.data, len(idx),
                                                 uvs.ctypes.data if len(idx) else dummy.ctypes.data, width, height, 1 if flip else 0,
                                                 C.byref(h)), "rayrs_lightmap_create")
        self._h = h
        n = C.c_uint64(0)
        _ffi.check(self._L.rayrs_lightmap_count(self._h, C.byref(n)), "rayrs_lightmap_count")
        self.n = int(n.value)

    @classmethod
    def from_object(cls, obj, uvs=None, cell: int = 8, gutter: int = 1, width: Optional[int] = None, height: Optional[int] = None,
                    flip: bool = False, device: int = 0) -> "Lightmap":
        """The atlas of a kind == "mesh" Object (or the one-element list Object.from_triangles returns).  uvs=None: every
        triangle gets its own texels (unwrap_triangles(m, cell, gutter)), and the atlas its size from that; with uvs, width and
        height are required."""
        if isinstance(obj, (list, tuple)) and len(obj) == 1:
            obj = obj[0]
        if not isinstance(obj, Object) or obj.kind != "mesh":
            raise ValueError('Lightmap.from_object takes an Object of kind "mesh"')
        if uvs is None:
            uvs, w, h = unwrap_triangles(len(obj.idx), cell, gutter)
            if (width is not None and int(width) != w) or (height is not None and int(height) != h):
                raise ValueError(f"the per-triangle unwrap of this mesh is {w} x {h}")
            width, height = w, h
        elif width is None or height is None:
            raise ValueError("with uvs, width and height are required")
        return cls(obj.verts, obj.idx, uvs, width, height, flip=flip, device=device)

    def _open(self, where):
        if self._h is None:
            raise _ffi.RayrsError(-1, where)  # a closed atlas
        return self._h

    @property
    def coverage(self) -> float:
        """The owned share of the atlas's texels."""
        return self.n / float(self.width * self.height)

    def _list(self, index=False, points=False, normals=False, bary=False):
        m = max(self.n, 1)
        out = [np.zeros(m, dtype=np.uint32) if index else None] + [np.zeros((m, 3)) if want else None for want in (points, normals, bary)]
        _ffi.check(self._L.rayrs_lightmap_texels(self._open("rayrs_lightmap_texels"), *[None if a is None else a.ctypes.data for a in out]),
                   "rayrs_lightmap_texels")
        return [None if a is None else a[:self.n] for a in out]

    def texels(self):
        """(index (n,) uint32 ascending: y * width + x, points (n, 3) f64, normals (n, 3) f64)."""
        index, points, normals, _ = self._list(index=True, points=True, normals=True)
        return index, points, normals

    def bary(self):
        """The barycentrics (b0, b1, b2) of the texels' centres in their owners, (n, 3) f64."""
        return self._list(bary=True)[3]

    def owner(self):
        """(H, W) int64: the triangle that owns each texel, -1 where none does."""
        out = np.zeros((self.height, self.width), dtype=np.uint32)
        _ffi.check(self._L.rayrs_lightmap_owner(self._open("rayrs_lightmap_owner"), out.ctypes.data), "rayrs_lightmap_owner")
        own = out.astype(np.int64)
        own[out == 0xFFFFFFFF] = -1
        return own

    def image(self, values, dilate: int = 2, return_valid: bool = False):
        """values (n,) or (n, C), C = 1 .. 4, one row per texel of texels() -> the (H, W, C) f64 image (a (n,) input: (H, W)):
        the rows at their texels, +0 elsewhere, then `dilate` rounds in which every texel without a value that has neighbours
        with one takes their mean.  return_valid: also the (H, W) bool plane of the texels that hold a value."""
        values = np.ascontiguousarray(values, dtype=np.float64)
        flat = values.ndim == 1
        if flat:
            values = values.reshape(-1, 1)
        if values.ndim != 2 or values.shape[0] != self.n or not 1 <= values.shape[1] <= 4:
            raise ValueError(f"values must be ({self.n},) or ({self.n}, C) with C = 1 .. 4")
        if int(dilate) < 0 or int(dilate) >= 2 ** 31:
            raise ValueError("dilate must be 0 .. 2^31 - 1")
        ch = values.shape[1]
        img, valid = np.zeros((self.height, self.width, ch)), np.zeros((self.height, self.width), dtype=np.uint8)
        if self.n == 0:
            values = np.zeros((1, ch))
        _ffi.check(self._L.rayrs_lightmap_assemble(self._open("rayrs_lightmap_assemble"), values.ctypes.data, ch, int(dilate), img.ctypes.data,
                                                   valid.ctypes.data), "rayrs_lightmap_assemble")
        if flat:
            img = img[:, :, 0]
        return (img, valid.astype(bool)) if return_valid else img

    def bake(self, scene: "Scene", **bake_args) -> "Bake":
        """Bake(scene, points, normals, kind="irradiance", **bake_args) at the atlas's texels; bake.values() then goes to image()."""
        if "kind" in bake_args:
            raise ValueError("a lightmap's bake is an irradiance bake")
        _, points, normals = self.texels()
        return Bake(scene, points, normals, kind="irradiance", **bake_args)

    def close(self):
        if self._h is not None:
            self._L.rayrs_lightmap_destroy(self._h)   # (no scene to outlive: the atlas owns all it frees)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- temporal accumulation (include/rayrs_hip.h TEMPORAL ACCUMULATION)

# Starting points, not tuned values: the weight a history pixel may carry into a blend, in samples (16 frames of 16); the
# relative depth difference and the distance of unit normals within which a tap of the history counts as the same surface.
TEMPORAL_MAX_SAMPLES = 256
TEMPORAL_DEPTH_TOL = 0.02
TEMPORAL_NORMAL_TOL = 0.25


def orbit(camera: Camera, degrees: float) -> Camera:
    """The camera turned by `degrees` about the axis through its lookat along its up (rayrs_camera_orbit: the same origin,
    to the bit, as the command line's --orbit builds)."""
    origin, up, lookat, fov, width, height, ppi = camera.args
    out = (C.c_double * 3)()
    st = _ffi.lib().rayrs_camera_orbit(_d3(origin), _d3(up), _d3(lookat), float(degrees), out)
    if st == -1:
        raise ValueError("rayrs_camera_orbit: invalid argument")
    _ffi.check(st, "rayrs_camera_orbit")
    return Camera(tuple(out), up, lookat, fov, width, height, ppi)


class History:
    """What earlier views of a static scene have seen, reprojected into each new view and blended with its frame
    (include/rayrs_hip.h TEMPORAL ACCUMULATION).  push(film) takes a film as it stands, on the device; image(),
    variance() and weight() read the history, denoised_guided() puts it through the variance-guided filter.  The defaults
    of max_samples, depth_tol and normal_tol are starting points (TEMPORAL_* above), as the filters' sigmas are."""

    def __init__(self, device: int = 0):
        self._L, self._h = _ffi.lib(), None
        self.camera, self.scene = None, None
        h = C.c_void_p()
        _ffi.check(self._L.rayrs_history_create(int(device), C.byref(h)), "rayrs_history_create")
        self._h = h

    def push(self, film: "Film", feature_samples: int = 16, max_samples: float = TEMPORAL_MAX_SAMPLES,
             depth_tol: float = TEMPORAL_DEPTH_TOL, normal_tol: float = TEMPORAL_NORMAL_TOL):
        """Blends the film's frame, with its noise plane and its tiles' sample counts as weights, into the history as seen
        from the film's camera.  The film is unchanged."""
        _ffi.check(self._L.rayrs_history_push_film(self._h, film._h, int(feature_samples), float(max_samples), float(depth_tol),
                                                   float(normal_tol)), "rayrs_history_push_film")
        self.camera, self.scene = film.camera, film.scene
        return self

    def push_image(self, camera: Camera, color, variance, weight, normal, albedo, depth, coverage, object,
                   max_samples: float = TEMPORAL_MAX_SAMPLES, depth_tol: float = TEMPORAL_DEPTH_TOL,
                   normal_tol: float = TEMPORAL_NORMAL_TOL):
        """The same with planes of the caller's, (H, W[, 3]) of the camera's size; albedo may be None."""
        color, (variance, weight, normal, albedo, depth, coverage) = _filter_inputs(
            color, [(variance, ()), (weight, ()), (normal, (3,)), (albedo, (3,)), (depth, ()), (coverage, ())], "plane", variance=True)
        H, W = color.shape[:2]
        obj = np.ascontiguousarray(object, dtype=np.uint32)
        if (H, W) != (camera.y_pixels(), camera.x_pixels()) or obj.shape != (H, W):
            raise ValueError(f"planes must be {(camera.y_pixels(), camera.x_pixels())}")
        if weight is None or normal is None or depth is None or coverage is None:
            raise ValueError("weight, normal, depth and coverage are required")
        _ffi.check(self._L.rayrs_history_push_image(self._h, C.byref(camera.desc), color.ctypes.data, variance.ctypes.data,
                                                    weight.ctypes.data, normal.ctypes.data, _ptr(albedo), depth.ctypes.data,
                                                    coverage.ctypes.data, obj.ctypes.data, float(max_samples), float(depth_tol),
                                                    float(normal_tol)), "rayrs_history_push_image")
        self.camera = camera
        return self

    def _shape(self):
        if self.camera is None:
            raise _ffi.RayrsError(-1, "rayrs_history_read")  # an empty history
        return self.camera.y_pixels(), self.camera.x_pixels()

    def read(self, out_f64: bool = True):
        """(colour, variance, weight) in one call."""
        H, W = self._shape()
        dt = np.float64 if out_f64 else np.float32
        c, v, m = np.zeros((H, W, 3), dtype=dt), np.zeros((H, W), dtype=dt), np.zeros((H, W), dtype=dt)
        _ffi.check(self._L.rayrs_history_read(self._h, 1 if out_f64 else 0, c.ctypes.data, v.ctypes.data, m.ctypes.data),
                   "rayrs_history_read")
        return c, v, m

    def image(self, out_f64: bool = False):
        H, W = self._shape()
        out = np.zeros((H, W, 3), dtype=np.float64 if out_f64 else np.float32)
        _ffi.check(self._L.rayrs_history_read(self._h, 1 if out_f64 else 0, out.ctypes.data, None, None), "rayrs_history_read")
        return out

    def variance(self):
        H, W = self._shape()
        out = np.zeros((H, W))
        _ffi.check(self._L.rayrs_history_read(self._h, 1, None, out.ctypes.data, None), "rayrs_history_read")
        return out

    def weight(self):
        H, W = self._shape()
        out = np.zeros((H, W))
        _ffi.check(self._L.rayrs_history_read(self._h, 1, None, None, out.ctypes.data), "rayrs_history_read")
        return out

    def push_times(self) -> dict:
        """HIP-event times of the last push(film), in milliseconds."""
        ms = (C.c_double * 5)()
        _ffi.check(self._L.rayrs_history_push_times(self._h, ms), "rayrs_history_push_times")
        return dict(zip(("features_ms", "read_ms", "noise_ms", "copy_ms", "reproject_ms"), ms))

    def denoised_guided(self, levels: int = 5, sigma_normal=SIGMA_NORMAL, sigma_albedo=SIGMA_ALBEDO, sigma_depth="scene",
                        sigma_luminance=SIGMA_LUMINANCE, out_f64: bool = False, return_variance: bool = False):
        """The history through the variance-guided filter (GUIDED FILTER) with the features of the view pushed last; sigmas
        as Film.denoised_guided -- sigma_depth="scene" is the default of the scene of the film pushed last, and no depth term
        after push_image."""
        if isinstance(sigma_depth, str):
            sigma_depth = scene_sigma_depth(self.scene) if self.scene is not None else None
        H, W = self._shape()
        out = np.zeros((H, W, 3), dtype=np.float64 if out_f64 else np.float32)
        out_var = np.zeros((H, W)) if return_variance else None
        _ffi.check(self._L.rayrs_history_denoise_guided(self._h, int(levels), _k(sigma_normal), _k(sigma_albedo), _k(sigma_depth),
                                                        _k(sigma_luminance), 1 if out_f64 else 0, out.ctypes.data, _ptr(out_var)),
                   "rayrs_history_denoise_guided")
        return (out, out_var) if return_variance else out

    def reset(self):
        _ffi.check(self._L.rayrs_history_reset(self._h), "rayrs_history_reset")
        self.camera = None

    def close(self):
        if self._h is not None:
            self._L.rayrs_history_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def render_sequence(scene: Scene, cameras, samples: int, sample_chunk: int = 4, history: Optional[History] = None,
                    feature_samples: int = 16, max_samples: float = TEMPORAL_MAX_SAMPLES, depth_tol: float = TEMPORAL_DEPTH_TOL,
                    normal_tol: float = TEMPORAL_NORMAL_TOL, **film_args):
    """For each camera: a film of `samples` samples, pushed into the history (a new one on the scene's device unless given).
    Yields (film, history) per camera, the history as it stands after that film's push; film_args go to Film()."""
    if history is None:
        history = History(device=int(scene._L.rayrs_scene_device(scene._h)))
    for camera in cameras:
        film = Film(scene, camera, sample_chunk=sample_chunk, **film_args)
        film.render(int(samples))
        history.push(film, feature_samples=feature_samples, max_samples=max_samples, depth_tol=depth_tol, normal_tol=normal_tol)
        yield film, history
