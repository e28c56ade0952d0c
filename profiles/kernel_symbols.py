#!/usr/bin/env python3
"""Do two builds of liblrp_hip.so hold the same device code?  No GPU needed.

  kernel_symbols.py A.so B.so      unbundles the gfx950 code object of each library and compares, kernel by kernel (mangled name),
                                   size and SHA-256 of the function's bytes; the order of the kernels in .text — which follows
                                   the order the host code instantiates the templates in — does not count.
  kernel_symbols.py A.so           lists name, size, digest

Listing of the commit that introduced conv_plan against its parent: conv_plan_ab.txt."""
import hashlib
import os
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
        out = {}
        for line in readelf("-sW"):
            f = line.split()
            if len(f) >= 8 and f[3] == "FUNC":
                a, n = int(f[1], 16), int(f[2])
                out[f[7]] = (n, hashlib.sha256(data[a - addr + off:a - addr + off + n]).hexdigest()[:16])
        return out


if __name__ == "__main__":
    a = kernels(sys.argv[1])
    if len(sys.argv) < 3:
        for k in sorted(a):
            print(k, *a[k])
        sys.exit(0)
    b = kernels(sys.argv[2])
    diff = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    print("%d / %d kernels, %d / %d bytes of code; kernels whose presence, size or bytes differ: %d" % (
        len(a), len(b), sum(v[0] for v in a.values()), sum(v[0] for v in b.values()), len(diff)))
    for k in diff:
        print("  ", k, a.get(k), b.get(k))
    sys.exit(1 if diff else 0)
