"""Stand-alone host programs of tests/native/ over the `__host__ __device__` headers of csrc/ (edge_model.h,
trust_region.h), built with g++ under AddressSanitizer + UndefinedBehaviorSanitizer as test_host_sanitizers.py builds its
program, and run as a process of their own."""
import os
import subprocess

import numpy as np

from conftest import ROOT

CSRC = os.path.join(ROOT, "toy-robust-backend-slam_amd", "csrc")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def _rocm_include():
    for d in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if d and os.path.exists(os.path.join(d, "include", "hip", "hip_runtime.h")):
            return os.path.join(d, "include")
    raise RuntimeError("hip/hip_runtime.h not found")


def build(tmp, name, sanitize=True):
    """g++ [-fsanitize=address,undefined] tests/native/<name>.cpp -> executable path.  sanitize=False: the plain program, for
    the tests that run where a GPU is (the sanitizer runs belong to the CPU tests)"""
    exe = os.path.join(str(tmp), name)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if sanitize else []
    cmd = ["g++", "-std=c++17", "-O1", "-g"] + san + ["-D__HIP_PLATFORM_AMD__", "-I" + _rocm_include(), "-I" + os.path.join(ROOT, "include"),
           "-I" + CSRC, os.path.join(ROOT, "tests", "native", name + ".cpp"), "-o", exe]
    subprocess.check_call(cmd)
    return exe


def run(args):
    p = subprocess.run(args, capture_output=True, text=True, timeout=300, env=ENV)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout


def edge_model(exe, tmp, P1, P2, meas, flags, phi=0.5):
    """edge_model_main on E edges -> (r_plain [E,3], J_plain [E,18], r_dcs [E,3], J_dcs [E,18])"""
    P1, P2, meas = (np.asarray(a, np.float64).reshape(-1, 3) for a in (P1, P2, meas))
    src, dst = os.path.join(str(tmp), "edges_in.txt"), os.path.join(str(tmp), "edges_out.txt")
    with open(src, "w") as f:
        for a, b, m, fl in zip(P1, P2, meas, flags):
            f.write(" ".join("%.17g" % v for v in (*a, *b, *m)) + " %d %.17g\n" % (int(fl), phi))
    out = run([exe, src, dst])
    assert "edge model ok: %d edges" % len(P1) in out
    v = np.loadtxt(dst, ndmin=2)
    assert v.shape == (len(P1), 42)
    return v[:, 0:3], v[:, 3:21], v[:, 21:24], v[:, 24:42]
