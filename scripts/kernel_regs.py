#!/usr/bin/env python3
"""print VGPR / SGPR / spill / LDS of every kernel in a hipcc -save-temps gfx950 .s file (the metadata YAML at its end)

    kernel_regs.py FILE.s [PATTERN]
    kernel_regs.py --unit NAME [PATTERN]     compile csrc/NAME.hip for gfx950 with -save-temps in a temporary directory first
                                             (e.g. --unit solver_chordal chordal: the rows of DESIGN.md section 4j)
"""
import os, re, subprocess, sys, tempfile


def rows(txt, pat):
    for blk in txt.split("  - .agpr_count:")[1:]:
        g = lambda k: (re.search(r"\.%s:\s+(\S+)" % k, blk) or [None, "?"])[1]
        name = g("name")
        if pat and not re.search(pat, name, re.I):
            continue
        print("%-90s vgpr %4s agpr %3s sgpr %3s spill %3s scratch %4s lds %6s" % (
            name.replace("_ZN3pgo3dev", "")[:90], g("vgpr_count"), blk.split()[0], g("sgpr_count"), g("vgpr_spill_count"),
            g("private_segment_fixed_size"), g("group_segment_fixed_size")))


if len(sys.argv) > 2 and sys.argv[1] == "--unit":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "toy-robust-backend-slam_amd", "csrc")
    with tempfile.TemporaryDirectory(prefix="kernel_regs_") as tmp:
        subprocess.check_call(["hipcc", "-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-Wno-unused-function", "-I" + os.path.join(root, "include"),
                               "-I" + csrc, "-save-temps", "-c", os.path.join(csrc, sys.argv[2] + ".hip"), "-o", "unit.o"], cwd=tmp)
        asm = [f for f in os.listdir(tmp) if f.endswith(".s") and "amdgcn" in f][0]
        rows(open(os.path.join(tmp, asm)).read(), sys.argv[3] if len(sys.argv) > 3 else "")
else:
    rows(open(sys.argv[1]).read(), sys.argv[2] if len(sys.argv) > 2 else "")
