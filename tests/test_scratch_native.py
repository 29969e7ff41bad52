"""csrc/scratch.h as a program of its own, tests/native/scratch_main.cpp, built by g++ under ASan + UBSan: the rule of the
layout (call order, disjoint regions, every region at a multiple of max(16, alignof(T)), bytes() a multiple of 16 that ends
the last region, empty spans for nothing, runs) over mixed element types and the counts 0, 1, 3, 15, 16, 17, and every element
of every region written and read back in a block of exactly bytes().  The header includes nothing of HIP: g++ takes it alone,
with no include path at all."""
import os
import re
import subprocess

import pytest

import _native_san as NS


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return NS.build(tmp_path_factory.mktemp("scratch_native"), "scratch_main")


def test_sanitized_layout_program_runs_clean(exe):
    out = NS.run([exe])
    m = re.search(r"scratch ok: (\d+) layouts, (\d+) checks", out)
    assert m, out
    assert int(m.group(1)) >= 6 * 2 * 6 * 2 and int(m.group(2)) > 10000


def test_header_is_plain_cxx17():
    src = '#include "%s"\n' % os.path.join(NS.CSRC, "scratch.h")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c++", "-"], input=src, text=True, check=True)
