#!/usr/bin/env python3
"""Do two builds of liblrp_hip.so hold the same device code?  No GPU needed.

  kernel_symbols.py A.so B.so      unbundles the gfx950 code object of each library and compares, kernel by kernel (mangled name),
                                   size and SHA-256 of the function's bytes; the order of the kernels in .text — which follows
                                   the order the host code instantiates the templates in — does not count.  For every kernel
                                   that differs it prints, for both builds, the resources the code object's metadata records:
                                   .vgpr_count, .sgpr_count, .private_segment_fixed_size (scratch bytes), .group_segment_fixed_size
                                   (LDS bytes), and marks a kernel that gained scratch or LDS or lost waves per SIMD.
  kernel_symbols.py A.so           lists name, size, digest

Listing of the commit that introduced conv_plan against its parent: conv_plan_ab.txt; of the split of the conv kernel's body:
conv_kernel_split_ab.txt."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")


def kernels(so):
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "dev.co")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, so])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat, "--output=" + co])
        readelf = lambda flag: subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), flag, co]).decode().splitlines()
        addr = off = None
        for line in readelf("-SW"):
            f = line.replace("[", " ").replace("]", " ").split()
            if len(f) > 4 and f[1] == ".text":
                addr, off = int(f[3], 16), int(f[4], 16)
        data = open(co, "rb").read()
        code = {}
        for line in readelf("-sW"):
            f = line.split()
            if len(f) >= 8 and f[3] == "FUNC":
                a, n = int(f[1], 16), int(f[2])
                code[f[7]] = (n, hashlib.sha256(data[a - addr + off:a - addr + off + n]).hexdigest()[:16])
        return code, resources("\n".join(readelf("--notes")), so)


RES_KEYS = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def resources(notes, so):
    """kernel -> the four figures of RES_KEYS, from amdhsa.kernels of the metadata note: one "  - " entry per kernel"""
    res = {}
    for entry in notes.split("\n  - ")[1:]:
        if ".vgpr_count:" not in entry:                    # (amdhsa.version is a list as well)
            continue
        fields = dict(re.findall(r"^\s*\.(\w+):\s+(\S+)", entry, re.M))
        missing = [k for k in ("name",) + RES_KEYS if k not in fields]
        if missing:
            sys.exit("%s: metadata entry of %s lacks %s" % (so, fields.get("name", "a kernel without .name"), ", ".join(missing)))
        res[fields["name"]] = tuple(int(fields[k]) for k in RES_KEYS)
    return res


def waves_per_simd(vgprs):
    """By the register file alone (gfx950: 512 VGPRs per SIMD lane, allocated in eights, 8 waves at most).  What a kernel really
    reaches is capped by its LDS and block size as well: a mark below means 'look', the record says what the look found."""
    return min(8, 512 // max(8, -(-vgprs // 8) * 8))


if __name__ == "__main__":
    a, res_a = kernels(sys.argv[1])
    if len(sys.argv) < 3:
        for k in sorted(a):
            print(k, *a[k])
        sys.exit(0)
    b, res_b = kernels(sys.argv[2])
    diff = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    print("%d / %d kernels, %d / %d bytes of code; kernels whose presence, size or bytes differ: %d" % (
        len(a), len(b), sum(v[0] for v in a.values()), sum(v[0] for v in b.values()), len(diff)))
    worse = 0
    for k in diff:
        print("  ", k, a.get(k), b.get(k))
        ra, rb = res_a.get(k), res_b.get(k)
        if ra and rb:
            bad = rb[2] > ra[2] or rb[3] > ra[3] or waves_per_simd(rb[0]) < waves_per_simd(ra[0])
            worse += bad
            print("       vgpr %d -> %d, sgpr %d -> %d, scratch %d -> %d, lds %d -> %d%s" % (
                ra[0], rb[0], ra[1], rb[1], ra[2], rb[2], ra[3], rb[3], "   <-- MORE scratch / LDS or fewer waves per SIMD" if bad else ""))
    if diff:
        print("kernels that gained scratch or LDS, or lost waves per SIMD: %d" % worse)
    sys.exit(1 if diff else 0)
