"""First-hit feature buffers and the feature-guided a-trous filter (include/rayrs_hip.h FEATURES, DENOISER) without a GPU:
the boundary's declarations and contract text, every refusal that is decided before the device is touched, the soundness
of the oracle-side references the GPU tests compare against (_features.py), the new kernels' resources from the ISA, and
the proof that no render changes: the ISA of every kernel of the four path translation units is the recorded one.

`python tests/test_features.py --record` rewrites tests/golden/path_kernels_isa.json from the tree as it stands (to be
done by a change that means to change a path kernel, never by one that does not)."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rayrs_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# the flags of rayrs_amd/csrc/Makefile's asm target
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-S",
         "--cuda-device-only"]
GOLDEN = os.path.join(ROOT, "tests", "golden", "path_kernels_isa.json")
PATH_UNITS = ("wavefront.hip", "local_pool.hip", "film.hip", "kernels.hip")
NEW_SYMBOLS = ["rayrs_render_features", "rayrs_film_features", "rayrs_film_denoise", "rayrs_image_denoise"]
# instructions no kernel of this library may name (scalar stores to memory and what goes with them), spelled in pieces
FORBIDDEN = ["s_" + "store_", "s_buffer_" + "store", "s_scratch_" + "store", "s_" + "atomic_", "s_buffer_" + "atomic", "s_dcache_" + "wb",
             "s_dcache_" + "discard"]


def compile_asm(source, out_dir):
    out = os.path.join(str(out_dir), source + ".s")
    subprocess.run([HIPCC, *FLAGS, "-o", out, source], cwd=CSRC, check=True, capture_output=True)
    return open(out).read()


def kernel_digests(asm):
    """sha256 of every kernel's code, from its label to the end of the function, as the compiler wrote it."""
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)", asm):
        name = m.group(1)
        body = re.search(rf"^{re.escape(name)}:.*?^\.Lfunc_end\d+:", asm, re.S | re.M)
        assert body, name
        out[name] = hashlib.sha256(body.group(0).encode()).hexdigest()
    return out


def kernel_resources(asm):
    res = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm, re.S):
        body = m.group(2)
        res[m.group(1)] = (int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1)),
                           int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)),
                           int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body).group(1)))
    return res


if __name__ == "__main__" and "--record" in sys.argv:
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        json.dump({u: kernel_digests(compile_asm(u, tmp)) for u in PATH_UNITS}, open(GOLDEN, "w"), indent=1, sort_keys=True)
    sys.exit(0)

import _features as F  # noqa: E402
import _film  # noqa: E402
import rayrs_amd  # noqa: E402
from rayrs_amd import _ffi, scenes  # noqa: E402


def header():
    return open(os.path.join(ROOT, "include", "rayrs_hip.h")).read()


# ------------------------------------------------------------------------------------------------------ the boundary

def test_the_header_declares_the_entry_points_with_their_contract():
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\bint {name}\s*\(", code), name
    text = re.sub(r"\s*\n \*\s*", " ", header())
    assert "e = ((dn*kn + da*ka) + dz*kz) + dc*kc_k" in text
    assert "w = (h[|dy|]*h[|dx|]) * rr_exp(-e)" in text
    assert "h[0] = 3/8, h[1] = 1/4, h[2] = 1/16" in text
    assert "kc_k = kc * 4^k" in text
    assert "the sum over s = 0 .. F-1 is SEQUENTIAL, in sample order, the first value assigned and the rest added" in text
    assert "sum * (1.0 / (double)F)" in text
    assert "NOT flipped towards the viewer" in text
    assert "A feature plane that is absent (NULL) contributes no term" in text


def test_the_library_exports_the_entry_points():
    L = _ffi.lib()
    for name in NEW_SYMBOLS:
        assert name in _ffi.SYMBOLS and hasattr(L, name), name
    for name in ("render_features", "denoise"):
        assert hasattr(rayrs_amd, name) and name in rayrs_amd.__all__
    assert hasattr(rayrs_amd.Film, "features") and hasattr(rayrs_amd.Film, "denoised")


def test_the_abi_version_and_the_layout_table_are_unchanged():
    L = _ffi.lib()
    assert L.rayrs_abi_version() == _ffi.ABI_VERSION == 7
    n = L.rayrs_abi_layout(None, 0)
    table = (C.c_uint32 * n)()
    assert L.rayrs_abi_layout(table, n) == n
    tail = []
    for st in (_ffi.FilmParams, _ffi.FilmStatus):
        tail += [C.sizeof(st), len(st._fields_)] + [getattr(st, name).offset for name, _ in st._fields_]
    assert list(table)[-len(tail):] == tail
    assert _ffi.ABI_STRUCTS[-2:] == [_ffi.FilmParams, _ffi.FilmStatus]


def test_integration_md_has_the_fn_lines():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"fn {name}\(", text), name


# ------------------------------------------------------------------------------------------------------ refusals

def host_scene_and_camera():
    cam_args, objs, heur, env = _film.sphere_desc()
    return rayrs_amd.Scene(objs, 1e-6, 1e6, heur, env, device=-1), rayrs_amd.Camera(*cam_args)


def test_feature_refusals_on_a_host_only_scene():
    L = _ffi.lib()
    scene, cam = host_scene_and_camera()
    n = cam.x_pixels() * cam.y_pixels()
    depth = np.zeros(n)

    def call(samples=16, rank=0, ranks=1, fast=0, scene_h=scene._h, camera=cam):
        return L.rayrs_render_features(scene_h, C.byref(camera.desc) if camera else None, samples, 7, rank, ranks, fast, None, None,
                                       depth.ctypes.data, None, None)

    assert call(scene_h=None) == -1 and call(camera=None) == -1
    assert call(samples=0) == -1
    assert call(samples=1 << 30) == -1
    assert call(fast=2) == -1
    assert call(rank=3, ranks=3) == -1 and call(rank=0, ranks=0) == -1
    big = rayrs_amd.Camera(*scenes.camera_for_resolution(_film.sphere_desc()[0], 70000, 8))
    assert call(camera=big) == -5
    assert call(samples=0, camera=big) == -1              # a parameter refusal comes first
    # everything in order: the scene has no device
    assert call() == -4
    assert call(samples=(1 << 30) - 1, rank=2, ranks=3, fast=1) == -4
    with pytest.raises(_ffi.RayrsError) as e:
        rayrs_amd.render_features(scene, cam)
    assert e.value.status == -4
    # the film's calls on no film
    assert L.rayrs_film_features(None, 16, None, None, depth.ctypes.data, None, None) == -1
    assert L.rayrs_film_denoise(None, 16, 5, 1.0, 1.0, 1.0, 1.0, 1, depth.ctypes.data) == -1


def test_denoise_refusals_before_the_device_is_touched():
    """device = -1 stands for "no device": every parameter refusal must come before RAYRS_NO_DEVICE."""
    L = _ffi.lib()
    color, out = np.zeros((4, 4, 3)), np.zeros((4, 4, 3))

    def call(levels=5, k=(1.0, 1.0, 1.0, 1.0), w=4, h=4, c=color, o=out):
        return L.rayrs_image_denoise(-1, w, h, c.ctypes.data if c is not None else None, None, None, None, levels, *k,
                                     o.ctypes.data if o is not None else None)

    assert call(levels=0) == -1 and call(levels=17) == -1
    for i in range(4):
        for bad in (-1.0, float("nan"), float("inf"), -0.5):
            k = [1.0] * 4
            k[i] = bad
            assert call(k=tuple(k)) == -1, (i, bad)
    assert call(c=None) == -1 and call(o=None) == -1 and call(w=0) == -1 and call(h=0) == -1
    assert call(w=70000, h=1) == -5 and call(w=1, h=65536) == -5
    assert call(w=70000, h=1, levels=0) == -1             # a parameter refusal comes first
    assert call() == -4 and call(levels=1, k=(0.0, 0.0, 0.0, 0.0)) == -4 and call(levels=16) == -4


def test_sigmas_become_reciprocal_squares():
    from rayrs_amd import api
    assert api._k(None) == 0.0 and api._k(float("inf")) == 0.0
    assert api._k(0.5) == 4.0 and api._k(0.1) == 1.0 / (0.1 * 0.1)
    for s in (None, float("inf"), 0.25, 0.6):
        assert api._k(s) == F.k_of(s)


# ------------------------------------------------------------------------------------------------------ the references

@pytest.mark.parametrize("name", ["sphere", "mesh"])
def test_the_feature_reference_is_sound(name):
    ps = F.named_samples(name, 5)
    f = F.features_from(ps, 5)
    h, w = f["depth"].shape
    hit = ps["coverage"] == 1.0
    assert hit.any() and ((ps["coverage"] == 0.0) | hit).all()
    lengths = np.sqrt((ps["normal"] ** 2).sum(axis=3))
    assert np.abs(lengths[hit] - 1.0).max() < 1e-14        # unit length to rounding
    assert (lengths[~hit] == 0.0).all()
    assert (f["coverage"] >= 0.0).all() and (f["coverage"] <= 1.0).all()
    assert (f["depth"] >= 0.0).all() and (ps["depth"][hit] > 0.0).all()
    assert ((f["object"] == F.MISS) == (ps["obj"][:, :, 0] < 0)).all()
    # a share: outside it +0 and the miss word, inside it the whole frame's values
    part = F.features_from(ps, 5, 1, 3)
    mask = rayrs_amd.tiles.tile_mask(w, h, 1, 3)
    assert (part["depth"][~mask] == 0.0).all() and (part["object"][~mask] == F.MISS).all()
    assert F.same_bits(part["normal"][mask], f["normal"][mask])
    # F = 1 is sample 0 itself
    one = F.features_from(ps, 1)
    assert F.same_bits(one["depth"], ps["depth"][:, :, 0]) and F.same_bits(one["normal"], ps["normal"][:, :, 0])


def test_the_centre_pixel_of_the_sphere_scene_sees_the_sphere():
    cam_args, objs, heur, env = _film.sphere_desc()
    flat = rayrs_amd.api.flatten_objects(objs)
    ps = F.named_samples("sphere", 5)
    f = F.features_from(ps, 5)
    k = int(f["object"][_film.H // 2, _film.W // 2])
    assert k != F.MISS and flat[k].kind == "sphere"
    assert f["coverage"][_film.H // 2, _film.W // 2] == 1.0
    assert tuple(f["albedo"][_film.H // 2, _film.W // 2]) == tuple(flat[k].mat.color)


def test_the_filter_reference_passes_nan_pixels_through_and_keeps_them_out_of_sums():
    color, normal, albedo, depth = F.random_case(3, 9, 7)
    k = (4.0, 25.0, 0.5, 1.0)
    out = F.atrous(color, normal, albedo, depth, 2, *k)
    bad = ~np.isfinite(color).all(axis=2)
    assert bad.sum() == 4
    assert F.same_bits(out[bad], color[bad])                 # passed through, NaN payloads and infinities included
    assert np.isfinite(out[~bad]).all()                      # and never in a neighbour's sum
    nan_feature = ~np.isfinite(normal).all(axis=2) & ~bad
    assert nan_feature.sum() == 2
    assert F.same_bits(out[nan_feature], color[nan_feature])  # den == 0: the pixel's own features are NaN
    # a neighbour's value does reach a finite pixel: changing one finite colour changes pixels around it
    other = color.copy()
    y, x = np.argwhere(~bad & ~nan_feature)[0]
    other[y, x] += 0.5
    changed = (F.atrous(other, normal, albedo, depth, 1, *k) != F.atrous(color, normal, albedo, depth, 1, *k)).any(axis=2)
    assert changed.sum() > 1
    # with every k zero and no NaN the filter is the B3-spline blur: constants stay constant
    flat = np.full((6, 6, 3), 0.25)
    assert np.abs(F.atrous(flat, None, None, None, 3, 0.0, 0.0, 0.0, 0.0) - 0.25).max() < 1e-15


# ------------------------------------------------------------------------------------------------------ the kernels

needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@needs_hipcc
def test_the_new_kernels_keep_their_occupancy_class(tmp_path):
    """the a-trous kernel 7 waves per SIMD (at most 72 registers) with no scratch and no LDS; the feature
    kernel 4 waves per SIMD on the compact layout (at most 128) and 3 on the f64 one (at most 168), its only LDS the
    traversal stacks it is launched with."""
    asm = compile_asm("features.hip", tmp_path)
    feats = kernel_resources(asm)
    assert len(feats) == 2 and all("features_kernel" in n for n in feats)
    atrous = {n: r for n, r in kernel_resources(compile_asm("denoise.hip", tmp_path)).items()
              if "atrous_kernel" in n and "guided_atrous_kernel" not in n}
    assert len(atrous) == 1
    for name, (vgpr, scratch, lds) in atrous.items():
        assert vgpr <= 72 and scratch == 0 and lds == 0, (name, vgpr, scratch, lds)
    for name, (vgpr, scratch, lds) in feats.items():
        bound = 128 if "features_kernelILb1E" in name else 168   # COMPACT
        assert vgpr <= bound and scratch == 0 and lds == 0, (name, vgpr, scratch, lds)
    low = asm.lower()
    for word in FORBIDDEN:
        assert word not in low, word


@needs_hipcc
@pytest.mark.parametrize("unit", PATH_UNITS)
def test_the_path_kernels_are_the_recorded_ones(unit, tmp_path):
    """No render changes: every kernel of the path translation units compiles to the ISA recorded before the features
    were added (tests/golden/path_kernels_isa.json)."""
    want = json.load(open(GOLDEN))[unit]
    got = kernel_digests(compile_asm(unit, tmp_path))
    assert sorted(got) == sorted(want)
    assert [n for n in want if got[n] != want[n]] == []
