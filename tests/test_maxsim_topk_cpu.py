"""CPU checks of ss_maxsim_topk's definition (tests/maxsim_topk_model.py) against the three consequences the header states, and
maxsim_topk_plan.hpp driven on the host under ASan + UBSan (tests/maxsim_topk_plan_harness.cpp)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import maxsim_model as mm
from tests import maxsim_topk_model as tm
from tests import vector_model as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spaghettisearch_amd", "csrc")
HIT_DTYPE = np.dtype([("doc", "<u4"), ("_pad", "<u4"), ("title", "<f8"), ("body", "<f8"), ("pagerank", "<f8"), ("final", "<f8")])
VEC = tm.VEC_HIT_DTYPE
FILL = 0xA5
LDS = 160 << 10


def filled(shape, dtype):
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return np.frombuffer(bytes([FILL]) * n, dtype=dtype).reshape(shape).copy()


# ---- the three consequences -----------------------------------------------------------------------------------------------------------

def test_known_world():
    tok_ptr, tok, qt_ptr, qtok = mm.known_world()
    hits, n = tm.topk(qt_ptr, qtok, tok_ptr, tok, 4, filled((1, 4), VEC), filled(1, np.int32))
    assert n.tolist() == [3] and hits[0, :3].tolist() == [(0, 16), (1, 12), (3, -11)]
    assert hits[0, 3:].tobytes() == bytes([FILL]) * 8                        # entries past the count untouched
    hits, n = tm.topk(qt_ptr, qtok, tok_ptr, tok, 1, filled((1, 1), VEC), filled(1, np.int32))
    assert n.tolist() == [1] and hits[0].tolist() == [(0, 16)]
    # an empty query: the first k docs that have a token, score 0
    hits, n = tm.topk(np.array([0, 0], np.uint32), None, tok_ptr, tok, 2, filled((1, 2), VEC), filled(1, np.int32))
    assert n.tolist() == [2] and hits[0].tolist() == [(0, 0), (1, 0)]
    # a mask of only the token-less doc: no row
    masks = np.array([[False, False, True, False], [False, True, True, True]])
    hits, n = tm.topk(np.array([0, 2, 2, 4], np.uint32), np.concatenate([qtok, qtok]), tok_ptr, tok, 4, filled((3, 4), VEC), filled(3, np.int32),
                      mask_id=[0, -1, 1], masks=masks)
    assert n.tolist() == [0, 3, 2] and hits[1, :3].tolist() == [(0, 0), (1, 0), (3, 0)] and hits[2, :2].tolist() == [(1, 12), (3, -11)]


@pytest.mark.parametrize("seed,k", [(31, 5), (32, 40), (33, 1)])
def test_rows_are_the_window_scores_sorted(seed, k):
    """consequence 1: ss_hit_maxsim_scores over all docs of the mask, sorted by (score desc, doc asc), rows without a score dropped"""
    rng = np.random.default_rng(seed)
    n_docs, dim, n_q = 30, 64, 4
    t_d = rng.integers(0, 6, n_docs)
    tok_ptr = np.zeros(n_docs + 1, np.uint64)
    tok_ptr[1:] = np.cumsum(t_d)
    tok = rng.integers(-3, 4, (int(tok_ptr[-1]), dim)).astype(np.int8)
    tok[:, 3:] = 0                                                           # few distinct scores: ties
    qt_ptr = np.array([0, 0, 2, 5, 6], np.uint32)
    qtok = rng.integers(-3, 4, (6, dim)).astype(np.int8)
    masks = rng.random((2, n_docs)) < 0.5
    mask_id = [-1, 0, 1, -1]
    got = tm.topk(qt_ptr, qtok, tok_ptr, tok, k, filled((n_q, k), VEC), filled(n_q, np.int32), mask_id=mask_id, masks=masks)
    for q in range(n_q):
        docs = [d for d in range(n_docs) if mask_id[q] < 0 or masks[mask_id[q]][d]]
        sc = mm.window_scores(qt_ptr, qtok, tok_ptr, tok, docs, q)
        want = sorted(((d, int(s)) for d, s in zip(docs, sc) if s != mm.NO_SCORE), key=lambda r: (-r[1], r[0]))[:k]
        assert got[1][q] == len(want) and got[0][q, :len(want)].tolist() == want
        assert got[0][q, len(want):].tobytes() == bytes([FILL]) * 8 * (k - len(want))


@pytest.mark.parametrize("k", [1, 7, 90, 200])
def test_one_token_tables_are_vector_topk(k):
    """consequence 2"""
    rng = np.random.default_rng(9)
    n_docs, dim, n_q = 90, 64, 5
    vec = rng.integers(-3, 4, (n_docs, dim)).astype(np.int8)
    vec[:, 6:] = 0
    qvec = rng.integers(-3, 4, (n_q, dim)).astype(np.int8)
    masks = rng.random((3, n_docs)) < 0.4
    masks[2] = False
    tok_ptr, qt_ptr = np.arange(n_docs + 1, dtype=np.uint64), np.arange(n_q + 1, dtype=np.uint32)
    for mask_id in (None, [0, -1, 1, 2, 0]):
        a = tm.topk(qt_ptr, qvec, tok_ptr, vec, k, filled((n_q, k), VEC), filled(n_q, np.int32), mask_id=mask_id, masks=masks)
        b = vm.topk(qvec, vec, k, filled((n_q, k), VEC), filled(n_q, np.int32), mask_id=mask_id, masks=masks)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ---- maxsim_topk_plan.hpp on the host -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("maxsim_topk_plan") / "maxsim_topk_plan_harness")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "maxsim_topk_plan_harness.cpp"), "-o", exe], check=True)
    return exe


def ask(harness, lines):
    r = subprocess.run([harness], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert out[-1] == f"ok {len(lines)} lines"
    return out[:-1]


def ptr(values):
    return f"{len(values) - 1} " + " ".join(str(v) for v in values)


INC, SLICE, FIXED = 64, 64, 256 * 4 + 16 * 4 + 1024 * 2


def per_query(qt, dim):
    """the token image at the padded stride, the joined maxima, threshold, count, mask id and m_q"""
    return 16 * qt * (dim + 16) + 16 * qt * 4 + 8 + 4 + 4 + 4


def block_model(dim, qt, k, n_q, limit):
    for qb in (16, 8, 4, 2, 1):
        if qb > 1 and n_q <= qb // 2:
            continue
        fixed = qb * per_query(qt, dim) + FIXED
        cap = (limit - fixed) // (qb * 8) if limit > fixed else 0
        if cap >= k + INC:
            cap = min(cap, max(2 * k, k + 4 * INC))
            return 1, qb, cap, fixed + qb * cap * 8
    return 0, 0, 0, 0


def test_plan_constants_match_the_sources():
    plan = open(os.path.join(CSRC, "maxsim_topk_plan.hpp")).read()
    assert int(re.search(r"SLICE_TOKENS = (\d+);", plan).group(1)) == SLICE
    assert int(re.search(r"GROUP_DOCS = (\d+);", plan).group(1)) == INC and "INC = GROUP_DOCS;" in plan
    assert '"maxsim.chunk_tokens"' in open(os.path.join(CSRC, "ctx.hip")).read()
    text = open(os.path.join(ROOT, "include", "spaghetti_rank.h")).read()
    assert "int32_t ss_maxsim_topk(ss_scorer* s, int32_t n_q," in text and "(A, 16), (B, 12), (D, -11)" in text


def test_plan_harness_query_blocks(harness):
    cases = [(dim, qt, k, n_q, LDS) for dim in (64, 128, 192, 1024) for qt in (1, 2, 4) for k in (1, 10, 100, 1000, 1024) for n_q in (1, 2, 3, 9, 1024)]
    out = ask(harness, ["b %d %d %d %d %d" % c for c in cases])
    assert out == ["%d %d %d %d" % block_model(*c) for c in cases]
    # dim 1024 with 64 tokens: one query's image alone is 66.5 KB, so two queries at the most; one in 100 KB; none in 64 KB
    assert 64 * 1040 == 66560
    assert ask(harness, [f"b 1024 4 1024 1024 {LDS}", f"b 1024 4 1 1024 {LDS}", "b 1024 4 1024 1024 100000", "b 1024 4 1 1024 65536"]) == [
        "1 2 1689 %d" % (2 * per_query(4, 1024) + FIXED + 2 * 1689 * 8), "1 2 257 %d" % (2 * per_query(4, 1024) + FIXED + 2 * 257 * 8),
        "1 1 2048 %d" % (per_query(4, 1024) + FIXED + 2048 * 8), "0 0 0 0"]
    # every seam: with exactly the bytes of qb queries at k + INC keys the block holds qb, with one byte less the next narrower one
    for dim, qt, k in ((128, 2, 100), (64, 1, 1024), (1024, 4, 10), (192, 4, 1)):
        for qb in (16, 8, 4, 2, 1):
            need = qb * per_query(qt, dim) + FIXED + qb * 8 * (k + INC)
            at, below = ask(harness, [f"b {dim} {qt} {k} 1024 {need}", f"b {dim} {qt} {k} 1024 {need - 1}"])
            assert at.split()[:3] == ["1", str(qb), str(k + INC)] and at.split()[3] == str(need)
            assert below.split()[:2] == (["1", str(qb // 2)] if qb > 1 else ["0", "0"])
    # a narrower block that holds every query is preferred; the tightest list a plan takes is k + INC
    assert [l.split()[1] for l in ask(harness, [f"b 128 2 10 {n} {LDS}" for n in (1, 2, 3, 4, 5, 8, 9, 16, 17)])] == \
        ["1", "2", "4", "4", "8", "8", "16", "16", "16"]
    assert ask(harness, [f"b 64 3 10 4 {LDS}", f"b 96 1 10 4 {LDS}", f"b 64 1 0 4 {LDS}", f"b 64 1 1025 4 {LDS}"]) == ["0 0 0 0"] * 4


def test_plan_harness_cut_tables(harness):
    cases = {
        (0,): "0",                                                           # zero docs
        (0, 0, 0): "0",                                                      # only token-less docs: no slice, no candidate
        (0, 1): "1 0 1",
        (0, 64): "1 0 1",
        (0, 65): "2 0 1 1",                                                  # one doc longer than a slice: the second slice is empty
        (0, 10, 310, 315): "5 0 2 2 2 2 3",                                  # ... three empty slices inside the long doc
        (0, 64, 64, 64, 128): "2 0 1 4",                                     # token-less docs stand with the doc that starts where they are
        (0, 0, 0, 64, 64, 64): "1 0 3",                                      # ... and those behind the table's last token in no slice
        (0, 5, 5, 5, 5): "1 0 1",
        (0, 32, 64, 96, 128, 129): "3 0 2 4 5",                              # docs ending exactly on a slice end
        (0, 63, 65, 127, 128): "2 0 2 4",
    }
    assert ask(harness, ["c " + ptr(v) for v in cases]) == list(cases.values())
    # against the definition: cut[s] is the first doc whose first token is at or behind token 64 s
    rng = np.random.default_rng(5)
    for _ in range(20):
        t = rng.choice([0, 0, 1, 3, 63, 64, 65, 200], rng.integers(1, 40))
        tp_ = [0] + np.cumsum(t).tolist()
        out = [int(x) for x in ask(harness, ["c " + ptr(tp_)])[0].split()]
        n_slices = -(-tp_[-1] // SLICE)
        assert out[0] == n_slices
        if n_slices:
            want = [min(d for d in range(len(tp_)) if tp_[d] >= s * SLICE) for s in range(n_slices)] + [max(d for d in range(1, len(tp_)) if tp_[d] > tp_[d - 1])]
            assert out[1:] == want


def chunks_model(n_slices, n_q, qb, k, opt, cu):
    nqb = -(-n_q // qb)
    if opt > 0:
        cs = -(-opt // SLICE)
    else:
        target = min(-(-4 * cu // max(nqb, 1)), max((256 << 20) // (max(n_q, 1) * k * 8), 1))
        cs = max(-(-n_slices // max(target, 1)), 4)
    nc = -(-n_slices // cs)
    return nqb, cs, nc


def test_plan_harness_chunks(harness):
    cases = [(n_slices, n_q, qb, k, opt, cu) for n_slices in (0, 1, 3, 4, 5, 1000, 1562500) for n_q, qb in ((1, 1), (40, 16), (1024, 16), (1024, 2))
             for k in (1, 100, 1024) for opt in (0, 1, 64, 65, 1000) for cu in (1, 256)]
    out = ask(harness, ["h %d %d %d %d %d %d" % c for c in cases])
    for c, line in zip(cases, out):
        ok, too_large, nqb, cs, nc, keys = (int(x) for x in line.split())
        assert (nqb, cs, nc) == chunks_model(*c), (c, line)
        if nc * c[3] > (1 << 37) // c[1]:                                    # the partial lists beyond 2^40 bytes: refused before the allocator
            assert (ok, too_large) == (0, 1) and c[4] > 0
            continue
        assert ok == 1 and too_large == 0 and keys == c[1] * nc * c[3]
        if c[4] == 0:
            assert keys * 8 <= (256 << 20) or cs == 4 or nc == 1              # the bound (a chunk is never below four slices, nor is there less than one)
    # the 256 MB bound shapes the default: 1024 queries at k = 1024 leave 32 chunks where the compute units would take 64
    assert ask(harness, ["h 1562500 1024 16 1024 0 1024"])[0].split()[4:] == ["32", str(1024 * 32 * 1024)]
    # more query blocks than a launch holds, and partial lists beyond 2^40 bytes
    assert ask(harness, ["h 100 65535 1 10 0 256"])[0].split()[0] == "1"
    assert ask(harness, ["h 100 65536 1 10 0 256"])[0].split()[:2] == ["0", "0"]
    assert ask(harness, [f"h {2 ** 17 + 1} 1024 16 1024 64 256"])[0].split()[:2] == ["0", "1"]
    assert ask(harness, [f"h {2 ** 17} 1024 16 1024 64 256"])[0].split()[:2] == ["1", "0"]
    assert ask(harness, [f"h {2 ** 40} 1 1 1 64 256"])[0].split()[:2] == ["0", "0"]     # more chunks than a launch holds


def test_plan_harness_chunks_cover_every_doc_once(harness):
    rng = np.random.default_rng(6)
    tables = [[0], [0, 0, 0], [0, 5], [0, 64, 128, 192], [0, 10, 310, 315], [0, 0, 0, 3, 3, 3 + 64 * 9, 3 + 64 * 9, 600, 600, 600]]
    for _ in range(12):
        t = rng.choice([0, 0, 1, 2, 5, 63, 64, 65, 300], rng.integers(1, 200))
        tables.append([0] + np.cumsum(t).tolist())
    lines, want_tokens = [], []
    for tp_ in tables:
        for opt in (0, 1, 64, 65, 128, 1000, 10 ** 9):
            for n_q, qb, k, cu in ((1, 1, 10, 256), (40, 16, 100, 256), (1024, 16, 1024, 4)):
                lines.append(f"v {opt} {n_q} {qb} {k} {cu} " + ptr(tp_))
                want_tokens.append((opt, max([b - a for a, b in zip(tp_, tp_[1:])], default=0)))
    out = ask(harness, lines)
    for line, (opt, longest), cmd in zip(out, want_tokens, lines):
        n_chunks, covered, max_tokens = (int(x) for x in line.split())
        assert covered == 1, (cmd, line)
        if opt > 0:                                                          # a forced chunk starts at most its size in tokens, plus the doc that runs over
            assert max_tokens < -(-opt // SLICE) * SLICE + max(longest, 1)
