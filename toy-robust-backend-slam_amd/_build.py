"""In-tree build of libpgo.so (hipcc, gfx950 only).  No JIT cache: the .so lives next to this
file so that it travels with the repository snapshot to the GPU box."""
from __future__ import annotations

import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
ROOT = os.path.dirname(HERE)
LIB = os.path.join(HERE, "libpgo.so")
SOURCES = ["host_graph.cpp", "structure.cpp", "comm.cpp", "knobs.cpp", "solver_create.hip", "solver_lm.hip", "solver_pcg.hip", "solver_direct.hip",
           "solver_batch.hip", "solver_abi.hip", "solver_launch.hip", "solver_covariance.hip", "solver_window.hip", "solver_score.hip", "solver_coarsen.hip", "solver_gnc.hip", "solver_support.hip", "solver_chordal.hip", "solver_mixture.hip", "solver_prior.hip"]
HEADERS = ["pgo_internal.h", "constants.h", "plan.h", "scratch.h", "comm.h", "loss.h", "gate.h", "edge_model.h", "trust_region.h", "kernels.hip.h", "solo.hip.h", "direct.hip.h", "coarse.hip.h", "covariance.hip.h", "sample.h", "sample.hip.h", "window.hip.h", "traj_error.h", "score.hip.h", "coarsen.h", "coarsen.hip.h", "gnc.h", "gnc.hip.h", "loop_support.h", "loop_support.hip.h", "chordal.h", "chordal.hip.h", "mixture.h", "mixture.hip.h", "prior.h", "prior.hip.h", "solver_handle.hip.h",
           os.path.join(ROOT, "include", "pgo.h")]


def _hipcc() -> str:
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: libpgo.so cannot be built (there is no CPU fallback)")


def needs_build() -> bool:
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, s) for s in SOURCES] + [h if os.path.isabs(h) else os.path.join(CSRC, h) for h in HEADERS]
    return any(os.path.getmtime(d) > t for d in deps)


def build_lib(force: bool = False, verbose: bool = False) -> str:
    if not force and not needs_build():
        return LIB
    # one object per translation unit, compiled side by side (the device code of a unit = the kernels it launches), then linked
    import tempfile
    from concurrent.futures import ThreadPoolExecutor
    flags = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-Wno-unused-function",
             "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
    with tempfile.TemporaryDirectory(prefix="pgo_build_") as tmp:
        def compile_one(src):
            obj = os.path.join(tmp, os.path.splitext(src)[0] + ".o")
            cmd = [_hipcc()] + flags + ["-c", os.path.join(CSRC, src), "-o", obj]
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.check_call(cmd)
            return obj
        with ThreadPoolExecutor(max_workers=min(len(SOURCES), max(1, (os.cpu_count() or 2) // 2))) as pool:
            objs = list(pool.map(compile_one, SOURCES))
        cmd = [_hipcc(), "--offload-arch=gfx950", "-fPIC", "-shared"] + objs + ["-o", LIB + ".tmp", "-lrccl", "-pthread"]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    os.replace(LIB + ".tmp", LIB)
    return LIB


def build_cli(force: bool = False) -> str:
    """The C++ host mirror of the reference's `main` (DATASET NUM_OUTLIER_LOOPS METHOD)."""
    out = os.path.join(HERE, "host", "main")
    src = os.path.join(HERE, "host", "main.cpp")
    if not os.path.exists(src):
        return ""
    hdrs = [os.path.join(HERE, "host", h) for h in os.listdir(os.path.join(HERE, "host")) if h.endswith(".h")]
    if (not force and os.path.exists(out) and
            all(os.path.getmtime(out) >= os.path.getmtime(p) for p in [src, LIB] + hdrs)):
        return out
    cmd = ["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(HERE, "host"), src,
           "-o", out, "-L" + HERE, "-lpgo", "-Wl,-rpath,$ORIGIN/..", "-Wl,-rpath," + HERE]
    subprocess.check_call(cmd)
    return out
