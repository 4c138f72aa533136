"""The lean walk of the PageRank work planner (plan_lean_items in spaghettisearch_amd/csrc/pr_plan.hpp) on its own, without a GPU:
tests/pr_lean_plan_harness.cpp is compiled with the host C++ compiler — no device header — under AddressSanitizer and UBSan.  The
lean table must be the dealt table without the items of dangling rows: every (wave, class) range in its own order (so a wave's
contribution sums are added in one order by both sweeps), offsets that count from `base`, two pad items at its end, and of a row cut
into pieces either every piece or none (a ticket is never left partially taken)."""
import os
import shutil
import subprocess
from collections import Counter

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spaghettisearch_amd", "csrc")
SEGW, WAVES, V_SEG, V_ZERO = 2048, 4, 8, 12
PAD = (V_ZERO, 0, 0, 0, 0, 0)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("pr_lean") / "pr_lean_plan_harness")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "pr_lean_plan_harness.cpp"), "-o", exe], check=True)
    return exe


def rle(degs):
    assert list(degs) == sorted(degs, reverse=True)
    vals, starts = [], []
    for i, d in enumerate(degs):
        if not vals or vals[-1] != d:
            vals.append(d)
            starts.append(i)
    return " ".join([str(len(vals))] + [f"{v} {s}" for v, s in zip(vals, starts)] + [str(len(degs))])


def plan(exe, nd, d, gw, nblocks, item_turns=4, base=0):
    text = f"{gw} {len(nd)} {nblocks} 128 {item_turns} {base}\n{rle(nd)}\n{rle(d)}\n"
    p = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    r = {"dealt": [], "lean": []}
    for line in p.stdout.split("\n"):
        f = line.split()
        if not f:
            continue
        if f[0] in ("dealt", "lean"):
            r[f[0]].append(tuple(int(x) for x in f[1:]))
        elif f[0] == "load":
            r["load"] = [float(x) for x in f[1:]]
        else:
            r[f[0]] = [int(x) for x in f[1:]]
    return r


def check(r, sl_nd, nblocks, base):
    dealt, lean, woff, loff = r["dealt"], r["lean"], r["woff"], r["loff"]
    nw = nblocks * WAVES
    n = len(dealt) - 2
    assert dealt[n:] == [PAD, PAD] and lean[-2:] == [PAD, PAD]
    m = len(lean) - 2
    assert len(woff) == len(loff) == nw * 8
    wb, lb = woff + [n], loff + [base + m]
    at = 0
    for j in range(nw * 8):
        want = [it for it in dealt[wb[j]:wb[j + 1]] if it[1] < sl_nd]          # the range's non-dangling items, in its order
        assert loff[j] == base + at
        assert lean[lb[j] - base:lb[j + 1] - base] == want
        at += len(want)
    assert at == m
    assert all(it[1] < sl_nd for it in lean[:m])
    assert Counter(lean[:m]) == Counter(it for it in dealt[:n] if it[1] < sl_nd)
    # rows cut into pieces: all pieces or none, and no piece of a dangling row
    pieces = Counter(it[1] for it in lean[:m] if it[0] == V_SEG)
    nseg = {it[1]: it[3] for it in dealt[:n] if it[0] == V_SEG}
    assert all(pieces[row] == nseg[row] for row in pieces)
    assert set(pieces) == {row for row in nseg if row < sl_nd}
    full_max, full_mean, lean_max, lean_mean = r["load"]
    assert lean_max <= full_max and lean_mean <= full_mean


ND = sorted([3 * SEGW + 1, 4097, 4096, 257, 256, 129, 128] + [17] * 9 + [16] * 70 + [9] * 5 + [8] * 40 + [5] * 33 + [4] * 70 + [3] * 65 + [2] * 130
            + [1] * 600 + [0] * 300, reverse=True)
DG = sorted([2 * SEGW + 1, 4097, 300, 257, 20, 9, 8, 8] + [2] * 50 + [1] * 10 + [0] * 20, reverse=True)
CASES = {"both_classes": (ND, DG),
         "no_dangling_rows": (ND, []),
         "dangling_rows_without_in_edges": (ND, [0] * 7),
         "only_dangling_rows": ([], DG),
         "only_dangling_destinations": ([0] * 300, DG),                # a bipartite graph: every in-edge ends in a dangling row
         "dangling_hub_in_pieces": ([5] * 40 + [0] * 10, [5 * SEGW + 3, 3 * SEGW, 4097]),
         "empty": ([], [])}


@pytest.mark.parametrize("base", [0, 100000])
@pytest.mark.parametrize("nblocks,item_turns", [(1, 1), (3, 4), (16, 8)])
@pytest.mark.parametrize("gw", [8, 16])
@pytest.mark.parametrize("name", list(CASES))
def test_lean_table_is_the_dealt_table_without_dangling_items(harness, name, gw, nblocks, item_turns, base):
    nd, d = CASES[name]
    r = plan(harness, nd, d, gw, nblocks, item_turns, base)
    check(r, len(nd), nblocks, base)
    n_lean = len(r["lean"]) - 2
    if name in ("no_dangling_rows", "dangling_rows_without_in_edges"):
        assert r["lean"] == r["dealt"] and r["loff"] == [v + base for v in r["woff"]]
    if name in ("only_dangling_rows", "empty"):
        assert n_lean == 0 and r["loff"] == [base] * len(r["loff"])
    if name == "only_dangling_destinations":
        assert n_lean > 0 and all(it[0] == V_ZERO for it in r["lean"])
    if name == "dangling_hub_in_pieces":
        assert sum(1 for it in r["dealt"] if it[0] == V_SEG) == 6 + 3 + 3 and not any(it[0] == V_SEG for it in r["lean"])
    if name == "both_classes":
        assert sum(1 for it in r["lean"] if it[0] == V_SEG) == 4 + 3 and sum(1 for it in r["dealt"] if it[0] == V_SEG) == 4 + 3 + 3 + 3
