"""CPU checks of the token-vector (MaxSim) definition (tests/maxsim_model.py): the header's hand-derived known answer, the numpy model
against a plain triple loop, the identity with tests/vector_model.py on one-token tables, and maxsim_plan.hpp driven on the host under
ASan + UBSan (tests/maxsim_plan_harness.cpp)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import maxsim_model as mm
from tests import vector_model as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spaghettisearch_amd", "csrc")
HIT_DTYPE = np.dtype([("doc", "<u4"), ("_pad", "<u4"), ("title", "<f8"), ("body", "<f8"), ("pagerank", "<f8"), ("final", "<f8")])
NO = mm.NO_SCORE
FILL = 0xA5


def filled(shape, dtype):
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return np.frombuffer(bytes([FILL]) * n, dtype=dtype).reshape(shape).copy()


def rows_of(rng, docs):
    docs = np.asarray(docs)
    hits = np.frombuffer(rng.bytes(docs.size * 40), dtype=HIT_DTYPE).reshape(docs.shape).copy()
    hits["doc"] = docs
    return hits


def loops(qt_ptr, qtok, tok_ptr, tok, q, d):
    """maxsim(q, d) with Python integers; None where the definition gives no score"""
    n_docs, dim = len(tok_ptr) - 1, qtok.shape[1] if len(qtok) else tok.shape[1]
    if d >= n_docs or tok_ptr[d + 1] == tok_ptr[d]:
        return None
    total = 0
    for i in range(int(qt_ptr[q]), int(qt_ptr[q + 1])):
        best = None
        for t in range(int(tok_ptr[d]), int(tok_ptr[d + 1])):
            s = 0
            for c in range(dim):
                s += int(qtok[i][c]) * int(tok[t][c])
            best = s if best is None or s > best else best
        total += best
    return total


# ---- the known answer of the header ---------------------------------------------------------------------------------------------------

def test_known_answer():
    tok_ptr, tok, qt_ptr, qtok = mm.known_world()
    assert [loops(qt_ptr, qtok, tok_ptr, tok, 0, d) for d in range(5)] == [16, 12, None, -11, None]
    hits = rows_of(np.random.default_rng(1), [[3, 2, 1, 0, 99]])            # D, C, B, A, doc 99
    n_hits = np.array([5], np.int32)
    sc = mm.hit_scores(qt_ptr, qtok, tok_ptr, tok, hits, n_hits, filled((1, 5), np.int32))
    assert sc[0].tolist() == [-11, NO, 12, 16, NO]
    got = mm.rerank(qt_ptr, qtok, tok_ptr, tok, hits, n_hits, 0, 5, filled((1, 5), HIT_DTYPE), filled(1, np.int32), filled((1, 5), np.int32))
    assert got[0]["doc"][0].tolist() == [0, 1, 3, 2, 99] and got[1].tolist() == [5] and got[2][0].tolist() == [16, 12, -11, NO, NO]
    assert got[0].tobytes() == hits[:, [3, 2, 0, 1, 4]].tobytes()           # the 40 bytes of a row, _pad included
    # a page out of the middle; entries past the count untouched
    got = mm.rerank(qt_ptr, qtok, tok_ptr, tok, hits, n_hits, 3, 4, filled((1, 4), HIT_DTYPE), filled(1, np.int32), filled((1, 4), np.int32))
    assert got[1].tolist() == [2] and got[0]["doc"][0, :2].tolist() == [2, 99] and got[0][0, 2:].tobytes() == bytes([FILL]) * 80
    # a query without tokens scores every doc that has a token 0
    sc = mm.hit_scores(np.array([0, 0], np.uint32), qtok, tok_ptr, tok, hits, n_hits, filled((1, 5), np.int32))
    assert sc[0].tolist() == [0, NO, 0, 0, NO]


# ---- the numpy model against loops ----------------------------------------------------------------------------------------------------

def random_world(seed, n_docs=25, dim=64, n_q=4, k_in=12, lo=-5, hi=6, max_t=7, max_m=5):
    rng = np.random.default_rng(seed)
    t_d = rng.integers(0, max_t + 1, n_docs)
    tok_ptr = np.zeros(n_docs + 1, np.uint64)
    tok_ptr[1:] = np.cumsum(t_d)
    tok = rng.integers(lo, hi, (int(tok_ptr[-1]), dim)).astype(np.int8)
    m_q = rng.integers(0, max_m + 1, n_q)
    m_q[0] = 0
    qt_ptr = np.zeros(n_q + 1, np.uint32)
    qt_ptr[1:] = np.cumsum(m_q)
    qtok = rng.integers(lo, hi, (int(qt_ptr[-1]), dim)).astype(np.int8)
    hits = rows_of(rng, rng.integers(0, n_docs + 3, (n_q, k_in)))            # some rows outside the table
    hits["doc"][:, 2] = hits["doc"][:, 9]                                   # the same doc twice
    n_hits = np.array([k_in, k_in - 5, 1, k_in][:n_q], np.int32)
    return tok_ptr, tok, qt_ptr, qtok, hits, n_hits


@pytest.mark.parametrize("seed", [21, 22, 23])
def test_model_equals_triple_loop(seed):
    tok_ptr, tok, qt_ptr, qtok, hits, n_hits = random_world(seed)
    tok[:, 4:] = 0                                                          # few distinct scores: ties inside every window
    n_q, k_in = hits.shape
    sc = mm.hit_scores(qt_ptr, qtok, tok_ptr, tok, hits, n_hits, filled((n_q, k_in), np.int32))
    got = mm.rerank(qt_ptr, qtok, tok_ptr, tok, hits, n_hits, 0, k_in, filled((n_q, k_in), HIT_DTYPE), filled(n_q, np.int32),
                    filled((n_q, k_in), np.int32))
    for q in range(n_q):
        n = int(n_hits[q])
        want = [loops(qt_ptr, qtok, tok_ptr, tok, q, int(d)) for d in hits["doc"][q, :n]]
        assert sc[q, :n].tolist() == [NO if w is None else w for w in want]
        assert sc[q, n:].tobytes() == bytes([FILL]) * 4 * (k_in - n)
        order = sorted(range(n), key=lambda j: (want[j] is None, 0 if want[j] is None else -want[j], j))
        assert got[1][q] == n and got[0][q, :n].tobytes() == hits[q, order].tobytes()
        assert got[2][q, :n].tolist() == [NO if want[j] is None else want[j] for j in order]


def test_model_extremes():
    """all -128 at dim 1024 and 64 query tokens: 2^30, the largest score; +127 against -128: the smallest"""
    tok_ptr = np.array([0, 3], np.uint64)
    tok = np.full((3, 1024), -128, np.int8)
    qt_ptr = np.array([0, 64], np.uint32)
    assert mm.maxsim(np.full((64, 1024), -128, np.int8), tok) == 2 ** 30
    assert mm.maxsim(np.full((64, 1024), 127, np.int8), tok) == -64 * 1024 * 127 * 128
    hits = rows_of(np.random.default_rng(3), [[0]])
    sc = mm.hit_scores(qt_ptr, np.full((64, 1024), -128, np.int8), tok_ptr, tok, hits, np.array([1], np.int32), filled((1, 1), np.int32))
    assert sc.tolist() == [[2 ** 30]]


# ---- one token per doc and per query: the doc-vector calls ----------------------------------------------------------------------------

@pytest.mark.parametrize("first,k", [(0, 40), (0, 7), (5, 10), (38, 5), (40, 3), (0, 1024)])
def test_one_token_tables_are_the_vector_calls(first, k):
    rng = np.random.default_rng(7)
    n_docs, dim, n_q, k_in = 90, 64, 5, 40
    vec = rng.integers(-3, 4, (n_docs, dim)).astype(np.int8)
    vec[:, 8:] = 0
    qvec = rng.integers(-3, 4, (n_q, dim)).astype(np.int8)
    hits = rows_of(rng, rng.integers(0, n_docs, (n_q, k_in)))
    hits["doc"][:, 5] = n_docs
    hits["doc"][:, 20] = 0xFFFFFFFF
    hits["doc"][:, 3] = hits["doc"][:, 11]
    n_hits = np.array([k_in, k_in - 7, 0, 1, k_in], np.int32)
    tok_ptr, qt_ptr = np.arange(n_docs + 1, dtype=np.uint64), np.arange(n_q + 1, dtype=np.uint32)
    a = mm.hit_scores(qt_ptr, qvec, tok_ptr, vec, hits, n_hits, filled((n_q, k_in), np.int32))
    b = vm.hit_scores(qvec, vec, hits, n_hits, filled((n_q, k_in), np.int32))
    assert a.tobytes() == b.tobytes()
    a = mm.rerank(qt_ptr, qvec, tok_ptr, vec, hits, n_hits, first, k, filled((n_q, k), HIT_DTYPE), filled(n_q, np.int32), filled((n_q, k), np.int32))
    b = vm.rerank(qvec, vec, hits, n_hits, first, k, filled((n_q, k), HIT_DTYPE), filled(n_q, np.int32), filled((n_q, k), np.int32))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- maxsim_plan.hpp on the host ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("maxsim_plan") / "maxsim_plan_harness")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "maxsim_plan_harness.cpp"), "-o", exe], check=True)
    return exe


def ask(harness, lines):
    r = subprocess.run([harness], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert out[-1] == f"ok {len(lines)} lines"
    return out[:-1]


def ptr_line(cmd, values):
    return f"{cmd} {len(values) - 1} " + " ".join(str(v) for v in values)


def test_plan_harness_query_tiles(harness):
    ms = [0, 1, 16, 17, 32, 33, 64]
    assert ask(harness, [f"q {m}" for m in ms]) == ["1", "1", "1", "2", "2", "4", "4"]
    # ... and through the pointer check: the largest m_q of a call chooses
    out = ask(harness, [ptr_line("p", [5, 5 + m]) for m in ms] + [ptr_line("p", [0, 3, 3, 36, 37]), ptr_line("p", [7])])
    assert out == [f"0 {m}" for m in ms] + ["0 33", "0 0"]
    # LDS: 16 QT padded rows and one maximum per wave and slot; the largest fits the device's 160 KB
    out = ask(harness, [f"l {qt} {dim}" for qt in (1, 2, 4) for dim in (64, 128, 1024)])
    want = [f"{dim + 16} {16 * qt * (dim + 16) + 4 * 16 * qt * 4}" for qt in (1, 2, 4) for dim in (64, 128, 1024)]
    assert out == want and 16 * 4 * 1040 + 1024 <= 160 << 10


def test_plan_harness_refusals(harness):
    INVALID, UNSUPPORTED = 1, 2
    assert ask(harness, [ptr_line("p", [0, 65])]) == [f"{UNSUPPORTED} 0"]              # 65 query tokens
    assert ask(harness, [ptr_line("p", [0, 64, 129])])[0].split()[0] == str(UNSUPPORTED)
    assert ask(harness, [ptr_line("p", [3, 2])])[0].split()[0] == str(INVALID)       # a decreasing pointer
    assert ask(harness, [ptr_line("p", [0, 70, 69])])[0].split()[0] == str(INVALID)  # decreasing beats too long
    assert ask(harness, [ptr_line("p", [1, 2])]) == ["0 1"]                           # qt_ptr need not start at 0
    tok = [(([0, 3, 3, 10]), 0), ([0], 0), ([1, 2], INVALID), ([0, 5, 4], INVALID), ([0, 2 ** 31 - 1], 0), ([0, 2 ** 31], UNSUPPORTED),
           ([0, 7, 7 + 2 ** 31, 2 ** 40], UNSUPPORTED), ([0, 2 ** 40, 5], INVALID)]
    assert ask(harness, [ptr_line("t", v) for v, _ in tok]) == [str(code) for _, code in tok]
    dims = [(64, 1), (128, 1), (1024, 1), (96, 0), (0, 0), (1088, 0), (-64, 0), (32, 0), (65, 0)]
    assert ask(harness, [f"d {d}" for d, _ in dims]) == [str(ok) for _, ok in dims]


def test_plan_harness_option_clamping(harness):
    plan = open(os.path.join(CSRC, "maxsim_plan.hpp")).read()
    default = int(re.search(r"DEFAULT_WIDE_TOKENS = (\d+);", plan).group(1))
    cases = [(0, default), (-7, default), (1, 1), (2, 2), (default, default), (2 ** 30, 2 ** 30), (2 ** 30 + 1, 2 ** 30), (2 ** 40, 2 ** 30)]
    assert ask(harness, [f"w {o}" for o, _ in cases]) == [str(v) for _, v in cases]


def test_plan_harness_grids(harness):
    cases = [(n_q, k_in, cu) for k_in in (1, 2, 3, 4, 5, 63, 64, 65, 100, 1000, 1024) for n_q in (1, 2, 7, 100, 1024, 5000) for cu in (1, 256)]
    out = ask(harness, [f"g {n_q} {k_in} {cu}" for n_q, k_in, cu in cases])
    for (n_q, k_in, cu), line in zip(cases, out):
        rows, per_q, n_wgs, ok, covered = (int(x) for x in line.split())
        assert ok == 1 and covered == 1, (n_q, k_in, cu, line)
        assert rows % 4 == 0 and 4 <= rows <= 64 and per_q == -(-k_in // rows) and n_wgs == n_q * per_q
        assert (per_q - 1) * rows < k_in                                      # no workgroup without a row
        if n_q * -(-k_in // 4) >= 4 * cu and k_in > 64:
            assert rows > 4                                                   # plenty of queries: long runs, the query tile loaded rarely
    # one query and a wide window: a workgroup per four rows; more workgroups than one launch holds: refused
    assert ask(harness, ["g 1 1024 256"])[0].split()[:2] == ["4", "256"]
    assert ask(harness, [f"g {2 ** 31} 1024 256"])[0].split()[3:] == ["0", "0"]
    assert ask(harness, [f"g {2 ** 27 - 1} 1024 256"])[0].split()[3] == "1"


def test_header_states_the_plan_constants():
    text = open(os.path.join(ROOT, "include", "spaghetti_rank.h")).read()
    plan = open(os.path.join(CSRC, "maxsim_plan.hpp")).read()
    assert int(re.search(r"#define SS_MAX_QUERY_TOKENS (\d+)", text).group(1)) == mm.MAX_QUERY_TOKENS
    assert int(re.search(r"MAX_QUERY_TOKENS = (\d+);", plan).group(1)) == mm.MAX_QUERY_TOKENS
    default = int(re.search(r"DEFAULT_WIDE_TOKENS = (\d+);", plan).group(1))
    assert f'"maxsim.wide_tokens" tokens (default {default})' in text
    assert '"maxsim.wide_tokens"' in open(os.path.join(CSRC, "ctx.hip")).read()
    from spaghettisearch_amd import _lib
    vp, i32 = _lib._vp, _lib._i32
    assert _lib.PROTOTYPES["ss_hit_maxsim_scores"][1] == [vp, i32, vp] + _lib.PROTOTYPES["ss_hit_vector_scores"][1][2:]
    assert _lib.PROTOTYPES["ss_rerank_hits_by_maxsim"][1] == [vp, i32, vp] + _lib.PROTOTYPES["ss_rerank_hits_by_vector"][1][2:]
    assert _lib.PROTOTYPES["ss_scorer_set_doc_tokens"][1] == [vp, i32, vp, vp]
