"""The resources of the bake's kernels, from the kernel metadata hipcc writes for gfx950 (no GPU needed).

bake.hip's wave kernels are radiance_direct_wave.h's wave, without and with the sky, with a third start (bake_kernels.h
BakeStart): they must keep what the waves have in radiance_direct.hip, radiance_sky.hip and film_direct.hip -- nothing in scratch,
and registers that allow two waves per SIMD (512 per lane and SIMD: at most 256 a wave).  Only the metadata is read."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rayrs_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# the flags of rayrs_amd/csrc/Makefile
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-S",
         "--cuda-device-only"]
VGPR_BOUND = 256


def kernel_resources(source, tmp_path):
    out = tmp_path / (source + ".s")
    subprocess.run([HIPCC, *FLAGS, "-o", str(out), source], cwd=CSRC, check=True, capture_output=True)
    res = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", out.read_text(), re.S):
        body = m.group(2)
        res[m.group(1)] = (int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1)),
                           int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)),
                           int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body).group(1)))
    return res


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_the_bake_kernels_use_no_scratch_and_keep_two_waves_per_simd(tmp_path):
    res = kernel_resources("bake.hip", tmp_path)
    direct = {n: r for n, r in res.items() if "bake_direct_kernel" in n}
    sky = {n: r for n, r in res.items() if "bake_sky_kernel" in n}
    small = {n: r for n, r in res.items() if n not in direct and n not in sky}
    # COMPACT x EXACT x {LIT_START_RAY, LIT_START_POINT} of either wave; accumulate, the select's three, status, noise, read
    assert len(direct) == 8 and len(sky) == 8 and len(small) == 7, sorted(res)
    for name, (vgpr, scratch, lds) in {**direct, **sky}.items():
        print(name, vgpr, scratch, lds)
        assert vgpr <= VGPR_BOUND and scratch == 0 and lds == 0, (name, vgpr, scratch, lds)   # (the stacks are dynamic LDS)
    for name, (vgpr, scratch, lds) in small.items():
        print(name, vgpr, scratch, lds)
        assert vgpr <= 64 and scratch == 0 and lds <= 64, (name, vgpr, scratch, lds)
