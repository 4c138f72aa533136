"""Learned ranking without a GPU: the numpy model (tests/rank_model_model.py) on the header's known answer and against a second,
recursive restatement on random forests; RankModel.flatten's pre-order; and rank_model_plan.hpp driven on the host under ASan + UBSan
(tests/rank_model_plan_harness.cpp): every refusal of ss_rank_model_create with its code, the model's figures, the packed node and the
cut of a forest into LDS chunks."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import rank_model_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spaghettisearch_amd", "csrc")
OK, INVALID, UNSUPPORTED = 0, 1, 2


def test_header_known_answer():
    m, x, want, order = rm.known_answer()
    got = rm.scores(m, x)
    assert got.tobytes() == want.tobytes()
    assert sorted(range(3), key=lambda j: (-got[j], j)) == order
    # ... and as a window: without a prox array every row's prox is absent (NaN goes right in T0), field 0 from a table
    hits = np.zeros((1, 3), dtype=[("doc", "<u4"), ("_pad", "<u4"), ("title", "<f8"), ("body", "<f8"), ("pagerank", "<f8"), ("final", "<f8")])
    hits["doc"], hits["final"] = [[0, 1, 2]], [[1.0, 1.5, 1.0]]
    fields = np.array([[50, rm.NO_FIELD_VALUE, 200]], dtype=np.int64)
    o_hits, o_n, o_sc = rm.rerank(m, hits, [3], 3, 0, 3, fields=fields)
    assert o_hits["doc"].tolist() == [[1, 0, 2]] and o_n.tolist() == [3] and o_sc.tolist() == [[4.75, 3.75, 3.25]]


def recursive_score(m, x):
    """the second restatement: recursion over a tree, math.fsum-free plain Python floats added in tree order"""
    def go(t, i):
        f, left, right, nan_left, value = (t[i][n].item() for n in ("feature", "left", "right", "nan_left", "value"))
        if f < 0:
            return value
        xv = float(x[f])
        return go(t, left if (nan_left == 1 if xv != xv else xv <= value) else right)
    acc = m["base"]
    if m["linear"] is not None:
        for w, xv in zip(m["linear"].tolist(), x.tolist()):
            if w != 0.0 and xv == xv:
                acc = acc + w * xv
    for t in m["trees"]:
        acc = acc + go(t, 0)
    return acc


@pytest.mark.parametrize("seed", range(4))
def test_model_against_recursion(seed):
    rng = np.random.default_rng(seed)
    nf = int(rng.choice([1, 15, 64]))
    trees = [rm.random_tree(rng, int(2 * rng.integers(0, 32) + 1), nf) for _ in range(int(rng.integers(0, 12)))]
    linear = None if seed % 2 else np.where(rng.random(nf) < 0.5, 0.0, rng.normal(size=nf))
    m = rm.model(nf, trees, linear, float(rng.normal()))
    x = rm.random_rows(rng, 40, nf)
    got = rm.scores(m, x)
    with np.errstate(all="ignore"):
        want = np.array([recursive_score(m, r) for r in x])
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    assert same.all()
    assert (got[np.isnan(got)].view(np.uint64) == rm.NAN_BITS).all()


def test_sum_order_matters():
    m = rm.model(1, [rm.tree(rm.leaf(1e16)), rm.tree(rm.leaf(1.0)), rm.tree(rm.leaf(-1e16))])
    assert rm.scores(m, [[0.0]]).tolist() == [0.0]            # (1e16 + 1.0 rounds to 1e16; any other order of the three gives 1.0)


def test_from_nested_flattens_in_preorder():
    from spaghettisearch_amd.engine import TREE_NODE_DTYPE, RankModel
    assert TREE_NODE_DTYPE == rm.TREE_NODE and TREE_NODE_DTYPE.itemsize == 24
    nested = {"f": 3, "thr": 0.5, "nan_left": True,
              "l": {"f": 1, "thr": -1.0, "l": {"leaf": 10.0}, "r": {"leaf": 20.0}},
              "r": {"f": 2, "thr": 7.0, "l": {"leaf": 30.0}, "r": {"f": 0, "thr": 0.0, "nan_left": 1, "l": {"leaf": 40.0}, "r": {"leaf": 50.0}}}}
    t = RankModel.flatten(nested)
    assert t.tolist() == [(3, 1, 4, 1, 0.5), (1, 2, 3, 0, -1.0), (-1, 0, 0, 0, 10.0), (-1, 0, 0, 0, 20.0), (2, 5, 6, 0, 7.0), (-1, 0, 0, 0, 30.0),
                          (0, 7, 8, 1, 0.0), (-1, 0, 0, 0, 40.0), (-1, 0, 0, 0, 50.0)]
    assert RankModel.flatten({"leaf": 2.5}).tolist() == [(-1, 0, 0, 0, 2.5)]
    x = np.array([np.nan, 0.0, 9.0, 2.0])                     # 2.0 > 0.5: right; 9.0 > 7.0: right; NaN: left
    assert rm.walk(t, x) == 40.0
    # a chain deeper than the interpreter's recursion limit would be: flatten does not recurse
    deep = {"leaf": 0.0}
    for i in range(3000):
        deep = {"f": 0, "thr": float(i), "l": deep, "r": {"leaf": 1.0}}
    d = RankModel.flatten(deep)
    assert len(d) == 6001 and (d["left"][d["feature"] >= 0] > np.flatnonzero(d["feature"] >= 0)).all()


# ---- rank_model_plan.hpp under the sanitizers ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("rank_model_plan") / "rank_model_plan_harness")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "rank_model_plan_harness.cpp"), "-o", exe], check=True)
    return exe


def ask(harness, lines):
    r = subprocess.run([harness], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert out[-1] == f"ok {len(lines)} lines"
    return out[:-1]


def model_line(nf, trees, linear=(), base=0.0, tree_ptr=None, n_trees=None):
    ptr, nodes = rm.flat([np.asarray(t, dtype=rm.TREE_NODE) for t in trees])
    ptr = ptr.tolist() if tree_ptr is None else list(tree_ptr)
    words = ["m", nf, repr(float(base)), len(linear), *[repr(float(w)) for w in linear], len(ptr) - 1 if n_trees is None else n_trees, *ptr, len(nodes)]
    for n in nodes:
        words += [n["feature"], n["left"], n["right"], n["nan_left"], repr(float(n["value"]))]
    return " ".join(str(w) for w in words)


STUMP = [rm.split(0, 0.5, 1, 2), rm.leaf(1.0), rm.leaf(2.0)]


def test_plan_harness_refusals(harness):
    s, l = rm.split, rm.leaf
    cases = [
        (model_line(2, [STUMP, [l(3.0)]], (0.5, 0.0), 1.0), OK),
        (model_line(1, []), OK),                                                     # n_trees = 0: a linear model
        (model_line(1, [], (np.inf,)), INVALID),                                     # a linear weight that is not finite
        (model_line(1, [], (np.nan,)), INVALID),
        (model_line(1, [], (), np.nan), INVALID),                                    # base
        (model_line(1, [], (), -np.inf), INVALID),
        (model_line(0, []), INVALID),                                                # n_features < 1
        (model_line(1, [], n_trees=-1, tree_ptr=[]), INVALID),                       # n_trees < 0
        (model_line(65, []), UNSUPPORTED),                                           # SS_MAX_RANK_FEATURES
        (model_line(64, []), OK),
        (model_line(1, [[l(0.0)]] * 8193), UNSUPPORTED),                             # SS_MAX_RANK_TREES
        (model_line(1, [[l(0.0)]] * 8192), OK),
        (model_line(1, [STUMP], tree_ptr=[1, 3]), INVALID),                          # tree_ptr does not start at 0
        (model_line(1, [STUMP, [l(0.0)]], tree_ptr=[0, 4, 3]), INVALID),             # decreases
        (model_line(1, [STUMP, [l(0.0)]], tree_ptr=[0, 3, 3, 4], n_trees=3), INVALID),   # an empty tree
        (model_line(1, [[l(0.0)]], tree_ptr=[0, (1 << 24) + 1]), UNSUPPORTED),       # more than 2^24 nodes (refused before a node is read)
        (model_line(2, [[s(2, 0.5, 1, 2), l(1.0), l(2.0)]]), INVALID),               # feature == n_features
        (model_line(2, [[s(1, 0.5, 1, 2), l(1.0), l(2.0)]]), OK),
        (model_line(2, [[(-2, 0, 0, 0, 0.0)]]), INVALID),                            # feature < -1
        (model_line(1, [[s(0, 0.5, 0, 2), l(1.0), l(2.0)]]), INVALID),               # left == own index
        (model_line(1, [[s(0, 0.5, 1, 0), l(1.0), l(2.0)]]), INVALID),               # right == own index
        (model_line(1, [[s(0, 0.5, 1, 2), s(0, 0.5, 0, 2), l(2.0)]]), INVALID),      # a child below its parent: a loop
        (model_line(1, [[s(0, 0.5, 3, 2), l(1.0), l(2.0)]]), INVALID),               # left == the tree's size
        (model_line(1, [[s(0, 0.5, 1, 3), l(1.0), l(2.0)]]), INVALID),               # right == the tree's size
        (model_line(1, [STUMP, [s(0, 0.5, 4, 5), l(1.0), l(2.0)]]), INVALID),        # children as indices of the whole array, not of the tree
        (model_line(1, [[s(0, 0.5, 1, 2, 2), l(1.0), l(2.0)]]), INVALID),            # nan_left > 1
        (model_line(1, [[s(0, np.nan, 1, 2), l(1.0), l(2.0)]]), INVALID),            # a NaN split value
        (model_line(1, [[s(0, np.inf, 1, 2), l(1.0), l(2.0)]]), OK),                 # ... an infinite one is a threshold like any other
        (model_line(1, [[s(0, 0.5, 1, 2), l(np.inf), l(2.0)]]), INVALID),            # a leaf value that is not finite
        (model_line(1, [[s(0, 0.5, 1, 2), l(1.0), l(np.nan)]]), INVALID),
        (model_line(1, [[s(0, 0.5, 1, 1), l(1.0), (7, 9, 9, 9, np.nan)]]), INVALID), # a node no walk reaches is checked too
        (model_line(1, [[s(0, 0.5, 1, 1), l(1.0)]]), OK),                            # both children the same leaf
    ]
    out = ask(harness, [c for c, _ in cases])
    assert [int(o.split()[0]) for o in out] == [code for _, code in cases]


def test_plan_harness_info(harness):
    rng = np.random.default_rng(5)
    chain = []                                                                       # a left-leaning chain of 70 splits
    for i in range(70):
        chain += [rm.split(0, float(i), 2 * i + 2, 2 * i + 1), rm.leaf(float(i))]
    chain.append(rm.leaf(-1.0))
    trees = [STUMP, [rm.leaf(1.0)], chain] + [rm.random_tree(rng, 2 * int(rng.integers(0, 32)) + 1, 3) for _ in range(5)]

    def depth(t, i=0):
        return 0 if t[i][0] < 0 else 1 + max(depth(t, int(t[i][1])), depth(t, int(t[i][2])))

    code, n_nodes, max_tree, max_depth = (int(w) for w in ask(harness, [model_line(3, trees)])[0].split())
    assert (code, n_nodes, max_tree) == (OK, sum(len(t) for t in trees), max(len(t) for t in trees))
    assert max_depth == max(depth(np.asarray(t, dtype=rm.TREE_NODE).tolist()) for t in trees) == 70
    assert ask(harness, [model_line(1, [[rm.leaf(1.0)]]), model_line(1, [])]) == ["0 1 1 0", "0 0 0 0"]
    # an unreachable chain behind a reachable stump does not count as depth
    assert ask(harness, [model_line(1, [[rm.split(0, 0.0, 1, 2), rm.leaf(0.0), rm.leaf(0.0), rm.split(0, 0.0, 4, 5), rm.split(0, 0.0, 5, 5), rm.leaf(0.0)]])]) == ["0 6 6 1"]


def test_plan_harness_links(harness):
    cases = [(0, 1, 2, 0), (63, (1 << 24) - 1, (1 << 24) - 2, 1), (14, 5, 9, 1), (-1, 123, 456, 1)]
    out = ask(harness, [f"p {f} {l} {r} {n}" for f, l, r, n in cases])
    assert out == ["0 0 1 2 0", f"0 63 {(1 << 24) - 1} {(1 << 24) - 2} 1", "0 14 5 9 1", "1 -1 0 0 0"]
    assert ask(harness, ["k 0", "k -5", "k 1", "k 16", "k 1024", "k 1025", f"k {1 << 40}"]) == ["1", "1", "1", "16", "1024", "1024", "1024"]


def chunks_of(harness, sizes, cap):
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(int).tolist()
    line = ask(harness, [" ".join(str(w) for w in ["c", cap, len(sizes), *ptr])])[0]
    cs = [tuple(int(v) for v in c.split(":")) for c in line.split()]
    # whole trees, in order, every tree once; a chunk's nodes are its trees'; oversize trees alone and marked, the others fit the cap;
    # a chunk is as long as the cap allows
    t = 0
    for i, (first, n, first_node, n_nodes, glob) in enumerate(cs):
        assert first == t and n >= 1 and first_node == ptr[first] and n_nodes == ptr[first + n] - ptr[first]
        assert glob == (n_nodes > cap) and (not glob or n == 1)
        if not glob and first + n < len(sizes):
            assert n_nodes + sizes[first + n] > cap
        t += n
    assert t == len(sizes)
    return cs


def test_plan_harness_chunks(harness):
    sizes = [7, 3, 1, 7, 7, 5]
    assert chunks_of(harness, sizes, 7) == [(0, 1, 0, 7, 0), (1, 2, 7, 4, 0), (3, 1, 11, 7, 0), (4, 1, 18, 7, 0), (5, 1, 25, 5, 0)]   # a tree's exact size
    assert chunks_of(harness, sizes, 6) == [(0, 1, 0, 7, 1), (1, 2, 7, 4, 0), (3, 1, 11, 7, 1), (4, 1, 18, 7, 1), (5, 1, 25, 5, 0)]   # one less
    assert [c[4] for c in chunks_of(harness, sizes, 1)] == [1, 1, 0, 1, 1, 1]                                                          # cap 1
    assert chunks_of(harness, sizes, 1024) == [(0, 6, 0, 30, 0)]
    assert chunks_of(harness, [1] * 9, 4) == [(0, 4, 0, 4, 0), (4, 4, 4, 4, 0), (8, 1, 8, 1, 0)]
    assert chunks_of(harness, [5, 2000, 5], 1024) == [(0, 1, 0, 5, 0), (1, 1, 5, 2000, 1), (2, 1, 2005, 5, 0)]
    assert chunks_of(harness, [], 16) == []
    rng = np.random.default_rng(2)
    for cap in (1, 2, 16, 63, 1024):
        chunks_of(harness, rng.integers(1, 64, size=300).tolist(), cap)
