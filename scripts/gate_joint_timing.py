"""Solver.gate_joint (pgo_edge_gate_joint) against Solver.gate (pgo_edge_gate) with the same arguments, in turns, and against what
the library offered for the sequential answer before: rounds of Solver.gate on the remaining candidates + Solver.set_active
after each acceptance.  INTEL + 50 (seed 1).  Medians of --rounds rounds (min .. max), milliseconds of wall time around calls
that end in a device synchronise.  Report only.  Run on the GPU box.

    python scripts/gate_joint_timing.py [--rounds 10]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import toy_robust_backend_slam_amd as P   # noqa: E402

DATA = os.path.join(ROOT, "tests", "golden", "data")
CHI2_95 = 7.814727903251179


def ms(call):
    t = time.perf_counter()
    out = call()
    return 1e3 * (time.perf_counter() - t), out


def in_turns(rounds, **calls):
    """every call once per round, in the order given; {name: (median, min, max)} and the last results"""
    t = {k: [] for k in calls}
    last = {}
    for k, c in calls.items():   # warm-up: code objects, the coarse level of a PCG call
        c()
    for _ in range(rounds):
        for k, c in calls.items():
            dt, last[k] = ms(c)
            t[k].append(dt)
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in t.items()}, last


def line(label, stat):
    print(f"| {label} | {stat[0]:.3f} ({stat[1]:.3f} .. {stat[2]:.3f}) |", flush=True)


def shape(value, call):
    P.set_knob("gate_joint_shape", value)
    try:
        return call()
    finally:
        P.set_knob("gate_joint_shape", -1)


def main(rounds):
    g = P.ReadG2O(os.path.join(DATA, "INTEL.g2o"))
    g.add_random_C(50, 1)
    E = g.n_edges - 50
    ia_g, ib_g, meas_g = np.array(g.ia), np.array(g.ib), np.array(g.meas)
    loops = np.nonzero(np.abs(ia_g - ib_g) != 1)[0]
    la, lb, lm = ia_g[loops], ib_g[loops], meas_g[loops]
    ba, bb, bm = ia_g[E:], ib_g[E:], meas_g[E:]
    s = P.Solver(g, P.Options(method=1, max_iters=5))
    s.solve()
    assert s.info().linear_solver == 2
    print(f"INTEL + 50, METHOD 1, {loops.size} loops; medians of {rounds} rounds (min .. max)\n\n| | ms |\n|---|---|")
    parts = [slice(0, 256), slice(256, loops.size)]
    st, _ = in_turns(rounds,
                     joint=lambda: [s.gate_joint(la[p], lb[p], lm[p], solver=1) for p in parts],
                     gate=lambda: [s.gate(la[p], lb[p], lm[p], solver=1) for p in parts])
    line(f"all {loops.size} loops, solver = 1: `pgo_edge_gate_joint`, calls of 256 + {loops.size - 256}", st["joint"])
    line("the same through `pgo_edge_gate`", st["gate"])
    for solver, kw in ((1, dict(solver=1)), (0, dict(poses_per_pass=16))):
        st, _ = in_turns(rounds if solver else max(2, rounds // 5),
                         joint=lambda: s.gate_joint(ba, bb, bm, **kw), gate=lambda: s.gate(ba, bb, bm, **kw))
        line(f"the 50 bogus loops, solver = {solver}: `pgo_edge_gate_joint`", st["joint"])
        line(f"the same through `pgo_edge_gate`", st["gate"])
    # the elimination at the cap, both shapes: 256 loops, everything forced in / everything rejected (no downdate)
    a, b, m = la[:256], lb[:256], lm[:256]
    one, zero = np.ones(256, np.int8), np.zeros(256, np.int8)
    st, last = in_turns(rounds,
                        b_in=lambda: s.gate_joint(a, b, m, force=one, solver=1), b_out=lambda: s.gate_joint(a, b, m, force=zero, solver=1),
                        a_in=lambda: shape(0, lambda: s.gate_joint(a, b, m, force=one, solver=1)),
                        a_out=lambda: shape(0, lambda: s.gate_joint(a, b, m, force=zero, solver=1)),
                        gate=lambda: s.gate(a, b, m, solver=1))
    line("n = 256, all forced in, (b) one launch per candidate (the library's shape)", st["b_in"])
    line("n = 256, all rejected, (b)", st["b_out"])
    line("n = 256, all forced in, (a) one launch of one workgroup (`gate_joint_shape` knob 0)", st["a_in"])
    line("n = 256, all rejected, (a)", st["a_out"])
    line("n = 256, `pgo_edge_gate`", st["gate"])
    for f in ("chi2_cond", "info_gain_cond", "P_cond"):
        assert np.array_equal(last["a_in"][1][f], last["b_in"][1][f]), f
    s.close()

    # the sequential answer before this call existed: METHOD 0, Trivial loss, the bogus edges inactive; Omega = I
    s = P.Solver(g, P.Options(method=0, max_iters=5, huber_delta=0.0))
    base = np.ones(g.n_edges, bool)
    base[E:] = False
    s.set_active(base)
    s.solve()
    poses = s.poses()
    kw = dict(solver=1) if s.info().linear_solver == 2 else dict(poses_per_pass=16)

    def rounds_of_gate(chi2_gate):
        """candidate k is judged after the accepted ones before it are residual blocks: gate the remaining ones, take the first
        that passes, activate it, gate what comes after it"""
        active, accepted, k0 = base.copy(), [], 0
        s.set_active(active)
        s.set_poses(poses)
        calls = 0
        while k0 < 50:
            out, _ = s.gate(ba[k0:], bb[k0:], bm[k0:], **kw)
            calls += 1
            ok = (out["status"] == 0) & (out["chi2_marginal"] <= chi2_gate) & (out["info_gain"] >= 0.0)
            if not ok.any():
                break
            k = k0 + int(np.argmax(ok))
            accepted.append(k)
            active[E + k] = True
            s.set_active(active)
            s.set_poses(poses)
            k0 = k + 1
        return accepted, calls

    def joint(chi2_gate):
        s.set_active(base)
        s.set_poses(poses)
        return s.gate_joint(ba, bb, bm, chi2_gate=chi2_gate, **kw)

    for gate_value in (CHI2_95, np.inf):
        st, last = in_turns(max(2, rounds // 2), joint=lambda: joint(gate_value), loop=lambda: rounds_of_gate(gate_value))
        acc_j = np.nonzero(last["joint"][1]["accepted"])[0].tolist()
        acc_l, calls = last["loop"]
        line(f"the 50 bogus loops, Trivial loss, {kw}, chi2_gate {gate_value:.4g}: one `pgo_edge_gate_joint` ({len(acc_j)} accepted)", st["joint"])
        # (the loop's P and gains are the joint call's; its chi2 is that of the residual at the poses, not moved by the accepted edges)
        line(f"{calls} x `pgo_edge_gate` on the rest + `pgo_set_active` after each acceptance ({len(acc_l)} accepted)", st["loop"])
    s.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    main(ap.parse_args().rounds)
