"""csrc/sample.h as a program of its own, tests/native/sample_main.cpp, built by g++ under ASan + UBSan: the run is clean, the
three Philox4x32-10 known answers hold, the uniforms stay inside (0, 1) at the all-zero and all-one words, the triple is what
its definition says, and the program's triples are those of the numpy restatement (tests/_sample_restatement.py)."""
import os

import numpy as np
import pytest

import _native_san as NS
import _sample_restatement as SR


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return NS.build(tmp_path_factory.mktemp("sample_native"), "sample_main")


def test_known_answers_uniform_ends_and_the_triple(exe):
    assert "sample ok" in NS.run([exe, "check"])


def test_restatement_has_the_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = SR.philox(np.array(ctr, np.uint64), np.array(key, np.uint64))
        assert tuple(int(v) for v in got) == want
    ends = SR.uniform(np.array([0, 0xffffffff], np.uint64), np.array([0, 0xffffffff], np.uint64))
    assert ends[0] == 2.0 ** -54 and ends[1] == 1.0 - 2.0 ** -53


def test_triples_match_the_restatement(exe, tmp_path):
    rng = np.random.default_rng(3)
    n = 4000
    seeds = [0, 1, 2 ** 32, 2 ** 64 - 1, 0x0123456789abcdef]
    rows = [(seeds[k % len(seeds)], k % 2, int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 2 ** 31))) for k in range(n)]
    rows += [(0, 0, 0, 0), (5, 1, 2 ** 32 - 1, 2 ** 31 - 1)]
    src, dst = os.path.join(str(tmp_path), "in.txt"), os.path.join(str(tmp_path), "out.txt")
    with open(src, "w") as f:
        f.write("%d\n" % len(rows))
        for r in rows:
            f.write("%d %d %d %d\n" % r)
    assert "sample triples ok: %d" % len(rows) in NS.run([exe, "triples", src, dst])
    got = np.loadtxt(dst, ndmin=2)
    for seed in set(r[0] for r in rows):
        for stream in (0, 1):
            sel = [k for k, r in enumerate(rows) if r[0] == seed and r[1] == stream]
            if sel:
                ref = SR.triples(seed, stream, [rows[k][2] for k in sel], [rows[k][3] for k in sel])
                assert np.abs(got[sel] - ref).max() <= 1e-14
