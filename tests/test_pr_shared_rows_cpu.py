"""The shared-row planner (plan_shared_rows in spaghettisearch_amd/csrc/pr_plan.hpp) on its own, without a GPU:
tests/pr_shared_rows_harness.cpp is compiled with the host C++ compiler — no device header — under AddressSanitizer and UBSan, and the
map from out-degree to table row is checked on empty input, a single degree, 100,000 distinct degrees and degrees far above the row count
(the sort path beside the flag path)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spaghettisearch_amd", "csrc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("pr_shared") / "pr_shared_rows_harness")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "pr_shared_rows_harness.cpp"), "-o", exe], check=True)
    return exe


def run(exe, pos_nd, od, ask=()):
    text = " ".join(map(str, [pos_nd, len(od), *od, len(ask), *ask])) + "\n"
    p = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    r = {}
    for line in p.stdout.split("\n"):
        f = line.split()
        if f:
            r[f[0]] = [int(x) for x in f[1:]]
    return r


def check(r, pos_nd, od, ask=()):
    distinct = sorted(set(od))
    assert r["table"] == [pos_nd + 1 + len(distinct), pos_nd, pos_nd + 1]
    assert r["deg"] == distinct
    where = {v: pos_nd + 1 + j for j, v in enumerate(distinct)}
    assert r["rows"] == [where[v] for v in od]                        # every row finds the shared row of its own degree ...
    assert all(pos_nd < x < r["table"][0] for x in r["rows"])        # ... inside the table, behind the zero row
    assert r["query"] == [where.get(v, pos_nd) for v in ask]          # a degree outside the map: the zero row


def test_empty_input(harness):
    for pos_nd in (0, 7):
        check(run(harness, pos_nd, [], [0, 1, 5]), pos_nd, [], [0, 1, 5])


def test_single_degree(harness):
    check(run(harness, 0, [3], [0, 2, 3, 4]), 0, [3], [0, 2, 3, 4])
    check(run(harness, 12, [1] * 50, [1, 2]), 12, [1] * 50, [1, 2])
    check(run(harness, 5, [4000000000], [4000000000, 4294967295, 0]), 5, [4000000000], [4000000000, 4294967295, 0])   # sort path, near 2^32


def test_the_benchmark_shape(harness):
    rng = np.random.default_rng(0)
    od = rng.choice(np.arange(1, 17), 5000, p=np.r_[0.75, 0.17, [0.08 / 14] * 14]).tolist()
    check(run(harness, 2388626, od, range(0, 20)), 2388626, od, range(0, 20))


@pytest.mark.parametrize("spread", [1, 40000])
def test_100000_distinct_degrees(harness, spread):
    """spread 1: degrees 1 .. 100,000 (flags per value); spread 40000: up to 4e9 (the largest far above the row count: sorted)"""
    rng = np.random.default_rng(spread)
    distinct = (1 + rng.permutation(100000)[:100000].astype(np.int64)) * spread - (spread - 1)
    od = np.concatenate([distinct, rng.choice(distinct, 30000)])
    rng.shuffle(od)
    od = od.tolist()
    assert len(set(od)) == 100000 and max(od) < 2 ** 32
    ask = [0, 2, max(od) + 1, od[0], od[-1]]
    check(run(harness, 1000, od, ask), 1000, od, ask)
