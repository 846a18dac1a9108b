#!/usr/bin/env python3
"""kernel_registers.py -- registers, LDS, scratch and spills of every kernel in the given objects, read from the code objects' metadata
the way the build's guard reads them (tools/isa_guard.py: code_object, kernel_meta).  Runs on the CPU.

usage: kernel_registers.py build/stress.o [build/mass.o ...] [--match k_stress]
One row per kernel: demangled name, VGPRs, SGPRs, static LDS bytes, scratch bytes, VGPR / SGPR spills and the waves per SIMD the
registers allow (512 VGPRs per SIMD lane, allocated in blocks of 8, at most 8 waves).  Exit status 1 if a listed kernel has scratch or spills."""
import argparse
import re
import sys
import tempfile

import isa_guard as ig


def plain_name(mangled: str) -> str:
    """k_name<ints> of a kernel template with integer arguments (all this project's are); anything else as it is."""
    m = re.search(r"\d+(k_\w+?)I((?:L[ib]\d+E)+)E", mangled)
    if not m:
        return mangled
    return m.group(1) + "<" + ",".join(re.findall(r"L[ib](\d+)E", m.group(2))) + ">"


def waves_per_simd(vgpr: int) -> int:
    return max(1, min(8, 512 // (((max(vgpr, 1) + 7) // 8) * 8)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("objects", nargs="+")
    ap.add_argument("--match", default="")
    ap.add_argument("--llvm", default=ig.LLVM)
    args = ap.parse_args()
    ig.LLVM = args.llvm
    bad = 0
    print("kernel\tvgpr\tsgpr\tlds_B\tscratch_B\tvspill\tsspill\twaves/SIMD")
    with tempfile.TemporaryDirectory() as tmp:
        for obj in args.objects:
            meta = ig.kernel_meta(ig.code_object(obj, tmp))
            names = sorted(n for n in meta if args.match in n)
            for n in names:
                m, d = meta[n], plain_name(n)
                print("\t".join(str(x) for x in (d, m.get("vgpr", -1), m.get("sgpr", -1), m.get("lds", -1), m.get("scratch", -1),
                                                 m.get("vspill", 0), m.get("sspill", 0), waves_per_simd(m.get("vgpr", 0)))))
                bad += bool(m.get("scratch", 0) or m.get("vspill", 0) or m.get("sspill", 0))
    if bad:
        sys.stderr.write(f"kernel_registers: {bad} kernels with scratch or spills\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
