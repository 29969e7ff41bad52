"""csrc/plan.h -- every choice a handle makes once, as pure functions of facts -- as a program of its own,
tests/native/plan_main.cpp, built by g++ under ASan + UBSan.  The program prints the decisions of a table of named cases, which
are compared here with answers derived by hand from the rules; it checks by itself that the partial arrays hold every product
grid (n_tiles 0 .. 70000), that the ranks of a world whose last rank owns no rows agree on the common side of the plan, and the
structural invariants of the launch code over a few thousand pseudo-random facts."""
import math
import os
import re
import subprocess

import pytest

import _native_san as NS

INVALID_ARG, UNSUPPORTED = -1, -8


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    return NS.run([NS.build(tmp_path_factory.mktemp("plan_native"), "plan_main")])


@pytest.fixture(scope="module")
def cases(out):
    res = {}
    for line in out.splitlines():
        if not line.startswith("case "):
            continue
        name = line.split()[1]
        d = dict(re.findall(r'(\w+)=("[^"]*"|\S*)', line))
        res[name] = {k: v.strip('"') for k, v in d.items()}
    return res


def ints(c, *keys):
    return tuple(int(c[k]) for k in keys)


def test_status_codes_are_the_abi_ones():
    text = open(os.path.join(NS.ROOT, "include", "pgo.h")).read()
    assert re.search(r"PGO_ERR_INVALID_ARG\s*=\s*-1\b", text) and re.search(r"PGO_ERR_UNSUPPORTED\s*=\s*-8\b", text)


def test_program_runs_clean_and_checks_its_invariants(out):
    m = re.search(r"sweep part_cap ok: (\d+) shapes", out)
    assert m and int(m.group(1)) > 4 * 70001, out[-600:]
    m = re.search(r"rank independence ok: (\d+) plans", out)
    assert m and int(m.group(1)) == 12
    m = re.search(r"random invariants ok: (\d+) plans, (\d+) refused", out)
    assert m and int(m.group(1)) > 2000
    assert re.search(r"plan ok: (\d+) checks", out)


def test_header_is_plain_cxx17():
    src = '#include "plan.h"\n'
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + NS.CSRC, "-I" + os.path.join(NS.ROOT, "include"),
                    "-x", "c++", "-"], input=src, text=True, check=True)


def test_product_kernel(cases):
    def form(name):
        c = cases[name]
        return c["spmv"], int(c["g_spmv"]), int(c["pad"])
    assert form("spmv_3") == ("p", 8, 0)
    assert form("spmv_4096") == ("p", 1024, 0)
    assert form("spmv_4097") == ("1", 4104, 1)
    assert form("spmv_4097_pipe2") == ("p", 1024, 1)
    assert form("spmv_4097_pipe0") == ("t", 2048, 1)
    assert form("spmv_3_pipe0") == ("t", 8, 0)
    assert form("spmv_3_pad1") == ("1", 8, 1)
    assert form("spmv_4097_pad0") == ("1", 4104, 0)
    for name in ("spmv_3_rows86", "spmv_3_inc257"):
        assert form(name)[:2] == ("t", 8)
    for name in ("spmv_4097_rows86", "spmv_4097_inc257"):
        assert form(name)[:2] == ("t", 2048)
    assert int(cases["part_cap_4097"]["part_cap"]) == 4624


def test_chain_apply(cases):
    shape = lambda n: ints(cases[n], "chunk", "steps", "nw", "scan", "g_chain")
    assert shape("chain_64_65536") == (2, 31, 1, 5, 512)
    assert shape("chain_64_65537") == (2, 31, 4, 0, 129)
    assert shape("chain_256_3500") == (4, 63, 1, 6, 14)
    assert shape("chain_32_1000") == (2, 15, 1, 0, 8)
    assert shape("chain_4_1000")[:4] == (2, 1, 1, 0)
    for n in (2, 6, 96, 512):
        c = cases["chain_bad_%d" % n]
        assert c["refused"] == "pre" and int(c["status"]) == INVALID_ARG
        assert c["why"] == "pcg_chain_len: a multiple of 4 that divides 256 (4 ... 256), 0 = off, -1 = auto"
    assert ints(cases["batch_chain_256"], "chunk", "steps", "solo_steps", "solo_scan") == (4, 63, 63, 6)
    assert ints(cases["batch_chain_64"], "chunk", "steps", "solo_steps", "solo_scan") == (4, 15, 15, 0)
    c = cases["batch_inc257"]
    assert c["refused"] == "shard" and int(c["status"]) == UNSUPPORTED and c["why"] == "pgo_batch: a problem has a row with more than 256 incidences"


def test_loop_form(cases):
    fused = lambda n: int(cases[n]["fused_p"])
    assert fused("fused_16384") == 1 and fused("fused_16385") == 0
    for n in ("fused_world2", "fused_force", "fused_batch", "fused_knob0"):
        assert fused(n) == 0, n
    assert fused("fused_coarse") == 0 and ints(cases["fused_coarse"], "coarse", "co_agg") == (1, 16)
    sr = lambda n: int(cases[n]["use_sr"])
    assert sr("sr_world2") == 1
    assert sr("sr_world2_tight") == 0
    assert sr("sr_world1") == 0
    assert sr("sr_world1_knob1_large") == 1 and fused("sr_world1_knob1_large") == 0
    assert sr("sr_world1_knob1_small") == 0 and fused("sr_world1_knob1_small") == 1   # the fused update wins
    assert sr("sr_world2_knob0") == 0
    assert sr("sr_world2_coarse") == 0 and int(cases["sr_world2_coarse"]["coarse"]) == 1


def test_reorder_and_alignment(cases):
    assert int(cases["reorder_world2"]["reorder"]) == 1
    assert int(cases["reorder_65537"]["reorder"]) == 1
    assert int(cases["reorder_65536"]["reorder"]) == 0
    assert int(cases["align_chain64_coarse48_world2"]["row_align"]) == 192
    assert int(cases["align_block4_coarse6_world2"]["row_align"]) == 12
    assert int(cases["align_chain64_coarse48_world1"]["row_align"]) == 64
    assert int(cases["align_chain64_coarse48_world2_batch"]["row_align"]) == 64
    c = cases["align_overflow"]
    assert c["refused"] == "pre" and int(c["status"]) == INVALID_ARG and c["why"] == "pcg_coarse_poses: too large to align the shards to"
    c = cases["align_at_limit"]
    assert c["refused"] == "none" and int(c["row_align"]) == 1 << 29


def test_coarse_level(cases):
    agg = lambda n: ints(cases[n], "coarse", "co_agg")
    assert agg("coarse_auto_511") == (0, 0)
    assert agg("coarse_auto_512") == (1, 16)
    assert agg("coarse_auto_8192") == (1, 16)
    assert agg("coarse_auto_8193") == (1, 64)
    assert agg("coarse_auto_131008") == (1, 64) and int(cases["coarse_auto_131008"]["co_K"]) == 6141
    assert agg("coarse_auto_131072") == (1, 128)
    for n in ("coarse_auto_loose", "coarse_auto_chain", "coarse_auto_block", "coarse_auto_direct", "coarse_auto_world2"):
        assert agg(n) == (0, 0), n
    assert int(cases["coarse_auto_direct"]["direct"]) == 1
    # ... where covariance calls can still build a level of their own, with the auto rule's aggregate size
    assert int(cases["coarse_auto_loose"]["cov_agg"]) == 16 and int(cases["coarse_auto_511"]["cov_agg"]) == 0
    c = cases["coarse_16_at_40000"]
    assert c["refused"] == "coarse" and int(c["status"]) == UNSUPPORTED
    assert c["why"] == "pcg_coarse_poses: the coarse matrix would have order 7500 (at most 6143)"
    c = cases["coarse_batch"]
    assert c["refused"] == "coarse" and int(c["status"]) == UNSUPPORTED and c["why"] == "pcg_coarse_poses: not inside a batched handle"
    for Kp in (32, 1024, 1056, 6112):
        c = cases["coarse_ndot_%d" % Kp]
        assert int(c["co_Kp"]) == Kp
        assert ints(c, "co_ndot", "co_explicit") == (((Kp + 3) // 4, 1) if Kp <= 1024 else ((Kp + 255) // 256, 0))


LADDER = [("world2", "one rank only"), ("force", "one rank only"), ("batch", "not inside a batched handle"), ("info", "not with information weighting"),
          ("no_constant", "needs a constant pose (it anchors the chain)"), ("permuted", "the internal pose ordering is on"),
          ("n1", "2 .. 65536 poses"), ("n65537", "2 .. 65536 poses"), ("gap", "poses 417 and 418 are not joined by an edge"),
          ("too_many", "2048 edges outside the odometry chain (at most 2047)"), ("all_at_once", "one rank only")]


@pytest.mark.parametrize("what,why", LADDER)
def test_direct_ladder(cases, what, why):
    c = cases["direct_auto_" + what]   # auto: silently PCG, no take-over
    assert c["refused"] == "none" and ints(c, "direct", "dl_possible") == (0, 0)
    c = cases["direct_forced_" + what]
    assert c["refused"] == "direct" and int(c["status"]) == UNSUPPORTED and c["why"] == "linear_solver = direct: " + why


def test_direct_choice(cases):
    for n in ("direct_auto_ok", "direct_forced_ok", "direct_auto_rtol_1e-8", "direct_auto_rank_2046", "direct_forced_rank_2049"):
        assert ints(cases[n], "direct", "dl_possible") == (1, 0), n
    for n in ("direct_auto_rtol_1e-7", "direct_auto_explicit_chain", "direct_auto_too_many"):
        assert ints(cases[n], "direct", "dl_possible") == (0, 0), n
    for n in ("direct_auto_rank_2049", "direct_takeover"):
        c = cases[n]
        assert ints(c, "direct", "dl_possible", "dl_K", "coarse") == (0, 1, 2049, 0)
        kk = 2049 / 5862.0
        assert float(c["dl_est"]) == pytest.approx(1.0e-3 + 11.7e-3 * kk * kk * math.sqrt(kk) + 0.15e-6 * 1000, rel=1e-14)
        assert ints(c, "dl_Kp", "dl_nsep", "dl_nseg") == (2080, 3, 32)   # sized once, for the take-over
    # the auto coarse level replaces the PCG / direct alternation
    assert ints(cases["direct_takeover_coarse_auto"], "direct", "dl_possible", "coarse", "co_agg") == (0, 0, 1, 16)
    c = cases["direct_bad_option"]
    assert c["refused"] == "direct" and int(c["status"]) == INVALID_ARG and c["why"] == "linear_solver: 0 = auto, 1 = PCG, 2 = direct (chain + low rank)"


def test_direct_sizes(cases):
    assert int(cases["direct_sizes_255"]["dl_nsep"]) == 0 and cases["direct_sizes_255"]["sep"] == ""
    c = cases["direct_sizes_256"]
    assert c["sep"] == "64/128/192"
    assert ints(c, "dl_K", "dl_Kp", "dl_nU", "dl_ld", "dl_seglen", "dl_nseg", "dl_fine", "dl_seglen2", "dl_nseg2") == (60, 64, 9, 128, 8, 32, 1, 1, 256)
    assert int(cases["direct_sizes_6000"]["dl_nsep"]) == 5
    assert int(cases["direct_sizes_65536"]["dl_nsep"]) == 15
    assert ints(cases["direct_sizes_4096"], "dl_fine", "dl_seglen2", "dl_nseg2") == (1, 16, 256)
    assert int(cases["direct_sizes_4097"]["dl_fine"]) == 0
