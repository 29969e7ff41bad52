"""The joint gate's elimination (csrc/gate.h, gate_joint_serial) as a program of its own, tests/native/gate_joint_main.cpp, built
by g++ once plainly and once under ASan + UBSan: both runs clean, both outputs the same text (g++ contracts nothing here), and
the records within the tolerance rule of test_gate_joint_host.py of the numpy elimination."""
import os

import numpy as np

import _native_san as NS
from test_gate_joint_host import CHI2_95, compare, eliminate, info_rows, problem, tolerances


def write_input(path, r, P, W, status, force, gate, gain):
    with open(path, "w") as f:
        f.write("%d %.17g %.17g\n" % (len(W), gate, gain))
        for k in range(len(W)):
            f.write("%d %d " % (status[k], force[k]) + " ".join("%.17g" % v for v in (*r[k], *info_rows(W)[k])) + "\n")
        for row in P:
            f.write(" ".join("%.17g" % v for v in row) + "\n")


def read_output(path, n):
    rows = [line.split() for line in open(path)]
    a = np.array([[float(v) for v in row] for row in rows[:n]])
    out = {"accepted": a[:, 0].astype(int), "status": a[:, 1].astype(int), "chi2_cond": a[:, 2], "info_gain_cond": a[:, 3], "r_cond": a[:, 4:7],
           "P_cond": a[:, 7:16].reshape(n, 3, 3)}
    return out, int(rows[n][0]), float(rows[n][1]), float(rows[n][2])


def test_plain_and_sanitized_programs(tmp_path):
    n = 12
    r, P, W = problem(n, 601)
    P[15:18, :] = 0.0          # candidate 5: between constant poses
    P[:, 15:18] = 0.0
    P[24:27, :] = 0.0          # candidate 8: not evaluable
    P[:, 24:27] = 0.0
    r[8] = np.nan
    status = np.zeros(n, int)
    status[8] = 1
    force = -np.ones(n, int)
    force[[2, 5, 8]] = 1
    force[3] = 0
    ref64 = eliminate(r, P, W, status, force)
    refld = eliminate(r, P, W, status, force, dtype=np.longdouble)
    src = os.path.join(str(tmp_path), "in.txt")
    write_input(src, r, P, W, status, force, CHI2_95, 0.0)
    text = []
    for sanitize in (False, True):
        exe = NS.build(tmp_path, "gate_joint_main", sanitize=sanitize)
        dst = os.path.join(str(tmp_path), "out_%d.txt" % sanitize)
        assert "gate joint ok: 12 candidates" in NS.run([exe, src, dst])
        text.append(open(dst).read())
        got, n_acc, chi2, gain = read_output(dst, n)
        compare(got, ref64, tolerances(ref64, refld, P), "sanitized" if sanitize else "plain")
        assert np.array_equal(got["accepted"], ref64["accepted"]) and got["status"].tolist() == status.tolist()
        assert got["accepted"][8] == 0 and got["accepted"][[2, 5]].tolist() == [1, 1] and got["accepted"][3] == 0
        assert n_acc == ref64["accepted"].sum() and 3 < n_acc < n
        acc = got["accepted"] == 1
        assert abs(chi2 - got["chi2_cond"][acc].sum()) <= n * np.finfo(float).eps * chi2
    assert text[0] == text[1]
