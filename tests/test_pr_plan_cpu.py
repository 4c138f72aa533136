"""The PageRank work planner (spaghettisearch_amd/csrc/pr_plan.hpp) on its own, without a GPU: tests/pr_plan_harness.cpp is compiled
with the host C++ compiler and no device header on the include path — that it compiles is the proof that the planner is host-only —
and its plans are checked against invariants on small constructed in-degree tables that hit every class boundary from both sides.
How level the deal ends up is a measured property, not an invariant, and is not asserted."""
import itertools
import os
import shutil
import subprocess
from collections import Counter

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spaghettisearch_amd", "csrc")
SEGW, CH, T_MULTI, T_DEG, WAVES = 2048, 16, 4096, 8, 4
W_SEG, W_WAVE, W_GROUP, W_ZERO, V_SEG, V_ROWW, V_QUAD, V_DEG, V_ZERO = 0, 1, 2, 3, 8, 9, 10, 11, 12
PAD = (V_ZERO, 0, 0, 0, 0, 0)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("pr_plan") / "pr_plan_harness")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-I", CSRC, os.path.join(ROOT, "tests", "pr_plan_harness.cpp"), "-o", exe],
                   check=True)
    return exe


def rle(degs):
    """falling degrees -> 'runs val start ... rows' as the harness reads it"""
    assert list(degs) == sorted(degs, reverse=True)
    vals, starts = [], []
    for i, d in enumerate(degs):
        if not vals or vals[-1] != d:
            vals.append(d)
            starts.append(i)
    return " ".join([str(len(vals))] + [f"{v} {s}" for v, s in zip(vals, starts)] + [str(len(degs))])


def plan(exe, nd, d, gw, lane_rows=0, nblocks=1, t_quad=128, item_turns=4, snake=-1, deal_global=2):
    text = f"plan {gw} {lane_rows} {len(nd)} {nblocks} {t_quad} {item_turns} {snake} {deal_global}\n{rle(nd)}\n{rle(d)}\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    r = {"item": [], "dealt": []}
    for line in out:
        f = line.split()
        if not f:
            continue
        if f[0] in ("item", "dealt"):
            r[f[0]].append(tuple(int(x) for x in f[1:]))
        else:
            r[f[0]] = [int(x) for x in f[1:]]
    return r


# every class boundary from both sides: the exact-degree classes R = 8 / 4 / 2 (1, 2 | 3, 4 | 5 .. 8), T_DEG (8, 9), one / two chunks
# (16, 17), T_QUAD of the two kernels (128, 129 and 256, 257), T_MULTI (4096, 4097), one hub of 3 SEGW + 1; runs long enough for more
# than one item per class; non-dangling rows without in-edges; a dangling class with and without in-edges
ND = sorted([3 * SEGW + 1, 4097, 4097, 4096, 4096, 257, 257, 256, 256, 129, 129, 128, 128] + [17] * 9 + [16] * 70 + [9] * 5 + [8] * 40 + [5] * 33
            + [4] * 70 + [3] * 65 + [2] * 130 + [1] * 600 + [0] * 300, reverse=True)
DG = sorted([4097, 300, 257, 20, 9, 8, 8] + [2] * 50 + [1] * 10 + [0] * 20, reverse=True)
GRAPHS = {"classes": (ND, DG), "dangling_edgeless": (ND, [0] * 7), "no_dangling": (ND, []), "empty": ([], []), "one_row": ([3], []),
          "one_edgeless_row": ([0], [])}


def check_cut(r, nd, d, gw, lane_rows, t_quad):
    """coverage, segments and class membership of the cut items; returns nothing"""
    sl_nd = len(nd)
    deg = lambda row: nd[row] if row < sl_nd else d[row - sl_nd]
    nslot = 64 // gw
    seg_w, multi_above = (SEGW, T_MULTI) if gw >= 8 else (128 * nslot, 32 * nslot)
    covered = Counter()
    hubs = {}
    for kind, row, count, nseg, sbase, tix in r["item"]:
        if kind in (V_SEG, W_SEG):
            assert deg(row) > multi_above
            hubs.setdefault(row, []).append((count, nseg, sbase, tix))
        elif kind == V_ROWW:
            assert t_quad < deg(row) <= T_MULTI
            covered[row] += 1
        else:
            rows = range(row, row + count)
            for q in rows:
                covered[q] += 1
                if kind == V_DEG:
                    assert deg(q) == nseg and 1 <= nseg <= T_DEG
                elif kind == V_QUAD:
                    assert (nseg - 1) * CH < deg(q) <= nseg * CH and T_DEG < deg(q) <= t_quad
                elif kind in (V_ZERO, W_ZERO):
                    assert deg(q) == 0 and q < sl_nd
                elif kind == W_WAVE:
                    assert 2 * nslot < deg(q) <= multi_above and count <= WAVES
                elif kind == W_GROUP:
                    assert 0 < deg(q) <= 2 * nslot
                else:
                    raise AssertionError(f"item kind {kind}")
    # a hub's pieces: indices 0 .. ns - 1 exactly once, ns from the cut's segment width, consecutive sbase, one ticket per hub
    next_sbase, tickets = 0, []
    for row in sorted(hubs):                       # rows rise with the table order: non-dangling hubs first
        pieces = hubs[row]
        ns = -(-deg(row) // seg_w)
        assert [p[0] for p in pieces] == list(range(ns))
        assert all(p[1] == ns and p[2] == next_sbase and p[3] == pieces[0][3] for p in pieces)
        next_sbase += ns
        if gw >= 8 or ns > 1:
            tickets.append(pieces[0][3])
        covered[row] += 1
    assert tickets == list(range(len(tickets)))
    nsegs, nmulti, seg_edges, pos_nd, pos_d = r["cut"]
    assert nsegs == next_sbase and nmulti == len(tickets) and seg_edges == 128 * nslot
    # every non-dangling row and every dangling row with in-edges in exactly one item; edge-less dangling rows in none
    want = {q for q in range(sl_nd)} | {sl_nd + q for q in range(len(d)) if d[q] > 0}
    if not want:
        assert r["item"] == [(W_ZERO, 0, 0, 0, 0, 0)]
    assert set(covered) == want and all(c == 1 for c in covered.values())
    assert pos_nd == sum(1 for x in nd if x > 0) and pos_d == sum(1 for x in d if x > 0)


def check_placement(r, nblocks):
    items, dealt, vbeg, woff = r["item"], r["dealt"], r["vbeg"], r["woff"]
    n = len(items)
    assert dealt[n:] == [PAD, PAD] and Counter(dealt[:n]) == Counter(items) and len(set(items)) == n
    nw = nblocks * WAVES
    assert len(woff) == nw * 8 and woff[0] == 0
    cls_of = lambda i: next((k for k in range(5) if i < vbeg[k + 1]), 5)
    index = {it: i for i, it in enumerate(items)}
    bounds = woff + [n]                            # wave-major: the range of (w, c) ends where the next one begins
    for w in range(nw):
        assert all(woff[8 * w + c] <= woff[8 * w + c + 1] for c in range(7))
        for c in range(8):
            lo, hi = bounds[8 * w + c], bounds[8 * w + c + 1]
            assert lo <= hi
            src = [index[it] for it in dealt[lo:hi]]
            assert all(cls_of(i) == c for i in src) and src == sorted(src)


BLOCK_CASES = [(name, gw) for name in GRAPHS for gw in (1, 2)]


@pytest.mark.parametrize("name,gw", BLOCK_CASES)
def test_block_items_cover_every_row_once(harness, name, gw):
    nd, d = GRAPHS[name]
    nslot = 64 // gw
    # k_pr_step's own thresholds from both sides: T_WAVE = 2 NSLOT, T_SEG = 32 NSLOT, one / two / four pieces of 128 NSLOT edges
    extra = [2 * nslot - 1, 2 * nslot, 2 * nslot + 1, 32 * nslot - 1, 32 * nslot, 32 * nslot + 1, 128 * nslot, 128 * nslot + 1, 3 * 128 * nslot + 1]
    nd2 = sorted(nd + extra, reverse=True) if nd else nd
    d2 = sorted(d + extra[:7], reverse=True) if d else d
    r = plan(harness, nd2, d2, gw)
    check_cut(r, nd2, d2, gw, 0, 128)
    assert not r["dealt"]


WAVE_CASES = [(name, gw, lane, dg, sn, nb, turns)
              for name, (gw, lane), dg, sn, nb, turns in itertools.product(GRAPHS, ((8, 0), (16, 0), (8, 1)), (0, 1, 2), (0, 1), (1, 3), (1, 64))]


@pytest.mark.parametrize("name,gw,lane_rows,deal_global,snake,nblocks,item_turns", WAVE_CASES)
def test_wave_items_are_cut_dealt_and_placed(harness, name, gw, lane_rows, deal_global, snake, nblocks, item_turns):
    nd, d = GRAPHS[name]
    t_quad = 256 if lane_rows else 128
    r = plan(harness, nd, d, gw, lane_rows, nblocks, t_quad, item_turns, snake, deal_global)
    check_cut(r, nd, d, gw, lane_rows, t_quad)
    check_placement(r, nblocks)


def test_default_snake_is_resolved_after_the_cut(harness):
    # "pr.deal_snake" unset: on for k_pr_sweep_n and from 8 items per wave on — both plans must still be valid
    for lane, nblocks in ((1, 3), (0, 1), (0, 3)):
        r = plan(harness, ND, DG, 8, lane, nblocks, 256 if lane else 128, 1, -1, 2)
        check_placement(r, nblocks)


def pack(exe, which, code):
    return int(subprocess.run([exe], input=f"{which} {code}\n", capture_output=True, text=True, check=True).stdout)


def test_class_orders_are_packed_position_by_position(harness):
    # 3 bits per position, first digit at position 0: 2-3-5-4-0-1
    assert pack(harness, "class_order", 235401) == 2 | 3 << 3 | 5 << 6 | 4 << 9 | 0 << 12 | 1 << 15 == 35162
    numbering = 0 | 1 << 3 | 2 << 6 | 3 << 9 | 4 << 12 | 5 << 15
    assert pack(harness, "class_order", 12345) == numbering == 181896
    assert pack(harness, "class_order", 112345) == numbering and pack(harness, "class_order", 7) == numbering
    # 2 bits per position: 2-3-1-0
    assert pack(harness, "n_order", 2310) == 2 | 3 << 2 | 1 << 4 | 0 << 6 == 30
    numbering4 = 0 | 1 << 2 | 2 << 4 | 3 << 6
    assert pack(harness, "n_order", 123) == numbering4 == 228
    assert pack(harness, "n_order", 1123) == numbering4 and pack(harness, "n_order", 7) == numbering4
