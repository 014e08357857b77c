"""Per-kernel comparison of the gfx950 code of two builds of the library's device objects (development aid).

usage: python scripts/kernel_disasm_diff.py [--objects a,b,c] OLD_DIR NEW_DIR [NAME ...]

OLD_DIR / NEW_DIR hold the objects to compare (default kernels.o, wavefront.o, local_pool.o and film.o; --objects names others,
e.g. ao,radiance,radiance_lit,radiance_direct,radiance_sky,film_direct,bake) of two builds (e.g. a copy of rayrs_amd/csrc/*.o made
before a change, and rayrs_amd/csrc after `make`).  Every kernel whose symbol contains one of NAME (default: the kernels
a render and rayrs_test_intersect run; `all`: every kernel of the objects) is disassembled from both builds and compared instruction by instruction, with
addresses, branch targets, pc-relative symbol offsets and the alignment padding behind a kernel's last instruction
normalised away.  Exit status 1 when one of them differs."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
OBJECTS = ("kernels", "wavefront", "local_pool", "film")
DEFAULT = ("wf_init", "wf_gen", "wf_trav", "wf_hit", "wf_miss", "lp_path", "test_intersect")


def disassemble(obj, tmp):
    fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "co")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True)
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", f"--input={fat}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}", "--unbundle"], check=True)
    text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co],
                          check=True, capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^<(.+)>:$", line.strip())
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        ins = line.split("//")[0].strip()
        if cur is None or not ins:
            continue
        ins = re.sub(r"<[^>]*>", "<L>", ins)
        prev = out[cur][-2:]
        if any(p.startswith("s_getpc_b64") for p in prev) and ins.startswith(("s_add_u32", "s_addc_u32")):
            ins = re.sub(r"0x[0-9a-f]+|-?\b\d+$", "<PCREL>", ins)  # the pc-relative offset of a symbol that moved
        out[cur].append(ins)
    for k in out:  # alignment padding behind the last s_endpgm belongs to where the next kernel starts
        while out[k] and out[k][-1] == "s_nop 0":
            out[k].pop()
    return out


def main():
    args, objects = sys.argv[1:], OBJECTS
    if args and args[0] == "--objects":
        objects, args = tuple(args[1].split(",")), args[2:]
    old_dir, new_dir = args[0], args[1]
    names = tuple(args[2:]) or DEFAULT
    same, differ = 0, []
    with tempfile.TemporaryDirectory() as tmp:
        for o in objects:
            a = disassemble(os.path.join(old_dir, o + ".o"), tmp)
            b = disassemble(os.path.join(new_dir, o + ".o"), tmp)
            for k in sorted(set(a) | set(b)):
                if "all" not in names and not any(n in k for n in names):
                    continue
                if a.get(k) == b.get(k):
                    same += 1
                else:
                    differ.append(k)
    for k in differ:
        print("differs:", k)
    print(f"{same} kernels identical, {len(differ)} differ")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
