"""CPU checks of ss_diversify_hits' definition (tests/diversify_model.py): the header's hand-derived known answer, the two identities the
definition implies (against tests/vector_model.py's re-rank), the vectorised model against a plain triple-loop walk, and
diversify_plan.hpp driven on the host under ASan + UBSan (tests/diversify_plan_harness.cpp)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import diversify_model as dm
from tests import vector_model as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spaghettisearch_amd", "csrc")
HIT_DTYPE = np.dtype([("doc", "<u4"), ("_pad", "<u4"), ("title", "<f8"), ("body", "<f8"), ("pagerank", "<f8"), ("final", "<f8")])
NO = dm.NO_SCORE
FILL = 0xA5


def filled(shape, dtype):
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return np.frombuffer(bytes([FILL]) * n, dtype=dtype).reshape(shape).copy()


def rows_of(rng, docs):
    docs = np.asarray(docs)
    hits = np.frombuffer(rng.bytes(docs.size * 40), dtype=HIT_DTYPE).reshape(docs.shape).copy()
    hits["doc"] = docs
    return hits


def run(qvec, vec, hits, n_hits, w_rel, w_div, first, k, info=True):
    n_q = hits.shape[0]
    return dm.diversify(qvec, vec, hits, n_hits, w_rel, w_div, first, k, filled((n_q, k), HIT_DTYPE), filled(n_q, np.int32),
                        filled((n_q, k), dm.INFO_DTYPE) if info else None)


# ---- the known answer of the header ---------------------------------------------------------------------------------------------------

def known_world():
    vec = np.zeros((4, 64), np.int8)
    vec[:, :2] = [(10, 0), (9, 1), (0, 8), (5, 5)]           # A, B, C, D
    qvec = np.zeros((1, 64), np.int8)
    qvec[0, 0] = 1
    hits = rows_of(np.random.default_rng(1), [[0, 1, 2, 3]])
    return vec, qvec, hits, np.array([4], np.int32)


def test_known_answer_sims_and_rel():
    vec, qvec, hits, _ = known_world()
    g = dm.gram(vec, [0, 1, 2, 3])
    assert (g[0, 1], g[0, 2], g[0, 3], g[1, 2], g[1, 3], g[2, 3]) == (90, 0, 50, 8, 50, 40) and (g == g.T).all()
    assert vm.scores(qvec, vec)[0].tolist() == [10, 9, 0, 5]


def test_known_answer_all_three_forms():
    vec, qvec, hits, n_hits = known_world()
    got = run(qvec, vec, hits, n_hits, 2, 1, 0, 4)
    assert got[0]["doc"][0].tolist() == [0, 2, 3, 1] and got[1].tolist() == [4]                   # A, C, D, B
    assert got[2][0].tolist() == [(10, NO), (0, 0), (5, 50), (9, 90)]
    assert got[0].tobytes() == hits[:, [0, 2, 3, 1]].tobytes()                                    # the 40 bytes of a row, _pad included
    got = run(qvec, vec, hits, n_hits, 1, 0, 0, 4)
    assert got[0]["doc"][0].tolist() == [0, 1, 3, 2]                                             # A, B, D, C
    got = run(None, vec, hits, n_hits, 30, 1, 0, 4)
    assert got[0]["doc"][0].tolist() == [0, 2, 1, 3]                                             # A, C, B, D
    assert got[2]["rel"][0].tolist() == [0, -2, -1, -3] and got[2]["sim"][0].tolist() == [NO, 0, 90, 50]
    # a page out of the middle, and entries past the count untouched
    got = run(qvec, vec, hits, n_hits, 2, 1, 1, 2)
    assert got[0]["doc"][0].tolist() == [2, 3] and got[2][0].tolist() == [(0, 0), (5, 50)]
    got = run(qvec, vec, hits, n_hits, 2, 1, 3, 4)
    assert got[1].tolist() == [1] and got[0]["doc"][0, 0] == 1 and got[0][0, 1:].tobytes() == bytes([FILL]) * 120


# ---- the identities -------------------------------------------------------------------------------------------------------------------

def random_world(seed, n_docs=90, dim=64, n_q=5, k_in=40, lo=-3, hi=4):
    rng = np.random.default_rng(seed)
    vec = rng.integers(lo, hi, (n_docs, dim)).astype(np.int8)
    qvec = rng.integers(lo, hi, (n_q, dim)).astype(np.int8)
    hits = rows_of(rng, rng.integers(0, n_docs, (n_q, k_in)))
    hits["doc"][:, 5] = n_docs                                 # outside the table
    hits["doc"][:, 20] = 0xFFFFFFFF
    hits["doc"][:, 3] = hits["doc"][:, 11]                     # the same doc twice
    n_hits = np.array([k_in, k_in - 7, 0, 1, k_in][:n_q], np.int32)
    return vec, qvec, hits, n_hits


@pytest.mark.parametrize("first,k", [(0, 40), (0, 7), (5, 10), (37, 3), (38, 5), (39, 3), (40, 3), (49, 3), (0, 1024)])
def test_zero_diversity_weight_is_the_rerank(first, k):
    vec, qvec, hits, n_hits = random_world(3)
    vec[:, 8:] = 0                                             # few distinct scores: ties inside every window
    n_q = hits.shape[0]
    want = vm.rerank(qvec, vec, hits, n_hits, first, k, filled((n_q, k), HIT_DTYPE), filled(n_q, np.int32), filled((n_q, k), np.int32))
    for w_rel in (1, 7, 65536):
        got = run(qvec, vec, hits, n_hits, w_rel, 0, first, k)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        for q in range(n_q):
            assert got[2]["rel"][q, :got[1][q]].tolist() == want[2][q, :want[1][q]].tolist()      # info.rel: the row's score


@pytest.mark.parametrize("first,k", [(0, 40), (3, 9), (37, 5), (40, 2)])
def test_by_rank_without_diversity_is_the_window_inside_rows_first(first, k):
    vec, _, hits, n_hits = random_world(4)
    n_docs, n_q = vec.shape[0], hits.shape[0]
    for w_rel in (0, 1, 65536):                                # (w_rel 0: every value ties, the smaller index wins: the same order)
        got = run(None, vec, hits, n_hits, w_rel, 0, first, k)
        for q in range(n_q):
            n = int(n_hits[q])
            docs = hits["doc"][q, :n]
            order = [j for j in range(n) if docs[j] < n_docs] + [j for j in range(n) if docs[j] >= n_docs]
            page = order[first:first + k]
            assert got[1][q] == len(page) and got[0][q, :len(page)].tobytes() == hits[q, page].tobytes()


# ---- the vectorised model against loops -----------------------------------------------------------------------------------------------

def brute(qvec_q, vec, docs, w_rel, w_div):
    """the whole walk of one window with Python integers -> [(window row, rel, pen at choice)], outside rows at the end"""
    n_docs, dim = vec.shape
    v = [[int(x) for x in row] for row in vec]
    inside = [j for j, d in enumerate(docs) if d < n_docs]
    outside = [j for j, d in enumerate(docs) if d >= n_docs]
    rel = {}
    for j in inside:
        rel[j] = -j if qvec_q is None else sum(int(qvec_q[t]) * v[docs[j]][t] for t in range(dim))
    chosen, out = [], []
    left = list(inside)
    while left:
        best = None
        for j in left:
            pen = 0
            for n_i, i in enumerate(chosen):
                s = 0
                for t in range(dim):
                    s += v[docs[i]][t] * v[docs[j]][t]
                pen = s if n_i == 0 else max(pen, s)
            value = w_rel * rel[j] - w_div * pen
            if best is None or value > best[0]:                # (left is ascending: the first of equal values stays)
                best = (value, j, pen)
        _, j, pen = best
        out.append((j, rel[j], pen if chosen else NO))
        chosen.append(j)
        left.remove(j)
    return out + [(j, NO, NO) for j in outside]


@pytest.mark.parametrize("seed,weights", [(11, (2, 1)), (12, (65536, 65536)), (13, (0, 1)), (14, (1, 0)), (15, (0, 0)), (16, (3, 5))])
def test_model_equals_triple_loop(seed, weights):
    rng = np.random.default_rng(seed)
    n_docs, dim, k_in = 30, 64, 14
    vec = rng.integers(-4, 5, (n_docs, dim)).astype(np.int8)
    vec[:, 6:] = 0                                             # small values: many equal sims and values
    qvec = rng.integers(-4, 5, (3, dim)).astype(np.int8)
    hits = rows_of(rng, rng.integers(0, n_docs + 4, (3, k_in)))   # some rows outside the table
    hits["doc"][:, 2] = hits["doc"][:, 9]
    n_hits = np.array([k_in, 9, 1], np.int32)
    for qv in (qvec, None):
        got = run(qv, vec, hits, n_hits, weights[0], weights[1], 0, k_in)
        for q in range(3):
            n = int(n_hits[q])
            want = brute(None if qv is None else qv[q], vec, [int(d) for d in hits["doc"][q, :n]], *weights)
            assert got[1][q] == n
            assert got[0][q, :n].tobytes() == hits[q, [j for j, _, _ in want]].tobytes()
            assert got[2][q, :n].tolist() == [(r, p) for _, r, p in want]


def test_model_value_edges():
    """all -128 at dim 1024: sim = 2^24 and value = -2^40 at the largest weight; the walk stays in int64"""
    vec = np.full((3, 1024), -128, np.int8)
    qvec = np.full((1, 1024), -128, np.int8)
    hits = rows_of(np.random.default_rng(2), [[0, 1, 2]])
    got = run(qvec, vec, hits, np.array([3], np.int32), 65536, 65536, 0, 3)
    assert got[0]["doc"][0].tolist() == [0, 1, 2] and got[2][0].tolist() == [(2 ** 24, NO), (2 ** 24, 2 ** 24), (2 ** 24, 2 ** 24)]
    assert dm.gram(vec, [0, 1])[0, 1] == 2 ** 24


# ---- diversify_plan.hpp on the host ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("diversify_plan") / "diversify_plan_harness")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "diversify_plan_harness.cpp"), "-o", exe], check=True)
    return exe


def ask(harness, lines):
    r = subprocess.run([harness], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert out[-1] == f"ok {len(lines)} lines"
    return out[:-1]


def test_plan_harness_groups_and_launches(harness):
    MB = 1 << 20
    cases = []
    for k_in, pitch in ((1, 64), (64, 64), (65, 128), (100, 128), (1000, 1024), (1024, 1024)):
        qb = pitch * pitch * 4
        for n_q in (1, 3, 17, 1024):
            # the default; exactly one query; one byte short of one; one byte short of two; exactly two; 17 queries; plenty; 1 byte
            for scratch in (0, qb, qb - 1, 2 * qb - 1, 2 * qb, 17 * qb, 1 << 40, 1):
                budget = 256 * MB if scratch < 1 else scratch
                group = max(1, min(budget // qb, n_q, 65535))
                cases.append((n_q, k_in, scratch, pitch, qb, group))
    cases.append((200000, 1, 1 << 40, 64, 16384, 65535))         # the grid's second dimension bounds a group
    cases.append((17, 1024, -5, 1024, 4 * MB, 17))               # a negative option: the default
    out = ask(harness, [f"g {n_q} {k_in} {scratch}" for n_q, k_in, scratch, _, _, _ in cases])
    for (n_q, k_in, scratch, pitch, qb, group), line in zip(cases, out):
        f = line.split()
        assert [int(x) for x in f[:5]] == [pitch, qb, group, -(-n_q // group), 1], (n_q, k_in, scratch, line)
        want = [f"{q}:{min(group, n_q - q)}" for q in range(0, n_q, group)]
        assert f[5:] == want
        if scratch >= qb:
            assert group * qb <= scratch                         # the scratch stays within the option
    # the issue's figure: 4 MB per query at k_in = 1024
    assert ask(harness, ["g 1024 1024 0"])[0].split()[:3] == ["1024", str(4 * MB), "64"]


def test_plan_harness_tile_pairs(harness):
    out = ask(harness, [f"t {t}" for t in range(1, 17)])
    for t, line in zip(range(1, 17), out):
        f = line.split()
        want = [f"{i}:{j}" for i in range(t) for j in range(i, t)]
        assert int(f[0]) == t * (t + 1) // 2 == len(want) and f[1:] == want


def test_plan_harness_checks(harness):
    cases = [((0, 0), 0), ((65536, 65536), 0), ((2, 1), 0), ((0, 65536), 0), ((-1, 0), 1), ((0, -1), 1), ((65537, 0), 1), ((0, 65537), 1),
             ((2 ** 31 - 1, 1), 1), ((1, -2 ** 31), 1)]
    out = ask(harness, [f"w {a} {b}" for (a, b), _ in cases])
    assert out == [str(code) for _, code in cases]


def test_plan_harness_keys(harness):
    rng = np.random.default_rng(5)
    cases = [(65536, 2 ** 24, 65536, -2 ** 24, 0), (65536, -2 ** 24, 65536, 2 ** 24, 1023), (0, 5, 0, 7, 0), (0, 5, 0, 7, 1023),
             (65536, 2 ** 24, 0, 0, 5), (0, 0, 65536, 2 ** 24, 5), (30, -1023, 1, 2 ** 24, 1023), (2, 10, 1, 0, 0)]
    for _ in range(200):
        cases.append((int(rng.integers(0, 65537)), int(rng.integers(-2 ** 24, 2 ** 24 + 1)), int(rng.integers(0, 65537)),
                      int(rng.integers(-2 ** 24, 2 ** 24 + 1)), int(rng.integers(0, 1024))))
    for _ in range(50):                                          # equal values: only the row decides
        cases.append((3, 100, 2, 50, int(rng.integers(0, 1024))))
    out = ask(harness, [" ".join(["k"] + [str(x) for x in c]) for c in cases])
    keyed = []
    for (w_rel, rel, w_div, pen, j), line in zip(cases, out):
        value, key, row = line.split()
        assert int(value) == w_rel * rel - w_div * pen and int(row) == j
        key = int(key, 16)
        assert 0 < key < 2 ** 53 and key == ((w_rel * rel - w_div * pen + 2 ** 42) << 10 | (1023 - j))
        keyed.append((key, w_rel * rel - w_div * pen, j))
    # descending keys = value descending, then row ascending
    assert sorted(keyed, key=lambda t: -t[0]) == sorted(keyed, key=lambda t: (-t[1], t[2]))
    assert max(abs(v) for _, v, _ in keyed) == 2 ** 41


def test_header_states_the_plan_constants():
    text = open(os.path.join(ROOT, "include", "spaghetti_rank.h")).read()
    plan = open(os.path.join(CSRC, "diversify_plan.hpp")).read()
    assert int(re.search(r"#define SS_DIV_WEIGHT_MAX (\d+)", text).group(1)) == dm.WEIGHT_MAX
    assert int(re.search(r"WEIGHT_MAX = (\d+);", plan).group(1)) == dm.WEIGHT_MAX
    from spaghettisearch_amd import _lib, engine
    assert _lib.SS_DIV_WEIGHT_MAX == dm.WEIGHT_MAX and engine.DIV_INFO_DTYPE == dm.INFO_DTYPE
    assert _lib.PROTOTYPES["ss_diversify_hits"][1] == _lib.PROTOTYPES["ss_rerank_hits_by_vector"][1][:6] + [_lib._i32] * 4 + [_lib._vp] * 3
