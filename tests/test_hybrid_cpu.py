"""CPU checks of hybrid search (ss_score_docs, ss_fuse_hits, ss_hybrid_topk): the numpy model against hand-derived
answers and against the oracle's ranking, the ABI's layouts through the host C compiler, the binding, and the host-only part of the
calls (spaghettisearch_amd/csrc/hybrid_plan.hpp) through tests/hybrid_plan_harness.cpp: a stand-alone program compiled with the host
C++ compiler, no device header on the include path, AddressSanitizer + UBSan."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from oracle import oracle_np
from tests import hybrid_model as hm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spaghettisearch_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "index_300x80.npz")
EMPTY = (np.zeros(2, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.float32))      # one term, no posting


def small_world(n_docs=100):
    return {"n_docs": n_docs, "title": EMPTY, "body": EMPTY, "mt": np.ones(n_docs), "mb": np.ones(n_docs), "prior": None}


def lists(lex_docs, vec_docs, finals=None, scores=None):
    lex = np.zeros((1, max(len(lex_docs), 1)), hm.HIT_DTYPE)
    lex["doc"][0, :len(lex_docs)] = lex_docs
    if finals is not None:
        lex["final"][0, :len(lex_docs)] = finals
    vec = np.zeros((1, max(len(vec_docs), 1)), hm.VEC_HIT_DTYPE)
    vec["doc"][0, :len(vec_docs)] = vec_docs
    if scores is not None:
        vec["score"][0, :len(vec_docs)] = scores
    return lex, np.array([len(lex_docs)], np.int32), vec, np.array([len(vec_docs)], np.int32)


def run_fuse(lex, n_lex, vec, n_vec, fp, first=0, k=16, world=None):
    world = world or small_world()
    vec_table = np.zeros((world["n_docs"], 64), np.int8)
    out = (np.zeros((1, k), hm.HIT_DTYPE), np.zeros(1, np.int32), np.zeros((1, k), hm.FUSED_DTYPE), np.zeros(1, np.int32))
    return hm.fuse(world, vec_table, np.array([0, 1], np.uint32), np.array([0], np.uint32), np.zeros((1, 64), np.int8), lex, n_lex, vec, n_vec,
                   fp, first, k, *out)


# ---- hand-derived answers -----------------------------------------------------------------------------------------------------------

def test_rrf_of_two_lists_with_one_shared_doc():
    hits, n, fused, n_union = run_fuse(*lists([10, 20, 30, 40], [50, 20, 60, 70]), (hm.FUSE_RRF, 60, 1.0, 1.0))
    # doc 20 stands second in both lists: 2 / 62; then the two firsts (1 / 61) by doc, the thirds (1 / 63), the fourths (1 / 64)
    assert n_union.tolist() == [7] and n.tolist() == [7]
    assert hits["doc"][0, :7].tolist() == [20, 10, 50, 30, 60, 40, 70]
    assert fused["score"][0, :7].tolist() == [1 / 62 + 1 / 62, 1 / 61, 1 / 61, 1 / 63, 1 / 63, 1 / 64, 1 / 64]
    assert fused["lex_rank"][0, :7].tolist() == [2, 1, 0, 3, 0, 4, 0] and fused["vec_rank"][0, :7].tolist() == [2, 0, 1, 0, 3, 0, 4]
    # the page: rows 2 .. 4 of that order, nothing behind them written
    hits, n, fused, _ = run_fuse(*lists([10, 20, 30, 40], [50, 20, 60, 70]), (hm.FUSE_RRF, 60, 1.0, 1.0), first=2, k=3)
    assert n.tolist() == [3] and hits["doc"][0].tolist() == [50, 30, 60]


def test_weighted_tie_is_broken_by_doc():
    lex, n_lex, vec, n_vec = lists([7, 3, 9], [3], finals=[5.0, 5.0, 4.0], scores=[1000])
    hits, n, fused, n_union = run_fuse(lex, n_lex, vec, n_vec, (hm.FUSE_WEIGHTED, 60, 1.0, 0.0))
    assert hits["doc"][0, :3].tolist() == [3, 7, 9] and fused["score"][0, :3].tolist() == [5.0, 5.0, 4.0]
    hits, n, fused, n_union = run_fuse(lex, n_lex, vec, n_vec, (hm.FUSE_WEIGHTED, 60, 2.0, 0.5))
    assert hits["doc"][0, :3].tolist() == [3, 7, 9] and fused["score"][0, :3].tolist() == [510.0, 10.0, 8.0]
    assert fused["vec_score"][0, :3].tolist() == [1000, 0, 0]           # docs 7 and 9: the zero table's score


def test_nan_final_lands_last_and_zeros_tie():
    lex, n_lex, vec, n_vec = lists([1, 2, 4, 3], [], finals=[np.nan, -1e300, np.nan, -0.0])
    vec2 = lists([], [0])[2]
    hits, n, fused, _ = run_fuse(lex, n_lex, vec2, np.array([1], np.int32), (hm.FUSE_WEIGHTED, 1, 1.0, -0.0))
    # w_vec = -0.0 keeps doc 3's -0.0 (-0.0 + -0.0); doc 0 (vector only, final 0.0 from an empty index: 0.0 + -0.0 = 0.0) ties it and
    # wins by doc; the NaN rows last, by doc
    assert hits["doc"][0, :5].tolist() == [0, 3, 2, 1, 4]
    bits = fused["score"][0, :5].view(np.uint64).tolist()
    assert bits == [0, 1 << 63, struct.unpack("<Q", struct.pack("<d", -1e300))[0], 0x7FF8000000000000, 0x7FF8000000000000]


def test_duplicated_doc_and_invalid_ids_keep_positions():
    lex, n_lex, vec, n_vec = lists([5, 5, 6, 1000, 8], [6, 4_000_000_000, 6, 5], finals=[1.0, 2.0, 3.0, 4.0, 5.0], scores=[9, 8, 7, 6])
    hits, n, fused, n_union = run_fuse(lex, n_lex, vec, n_vec, (hm.FUSE_RRF, 1, 1.0, 1.0))
    assert n_union.tolist() == [3]
    by_doc = {int(h["doc"]): (int(f["lex_rank"]), int(f["vec_rank"]), float(h["final"]), int(f["vec_score"]))
              for h, f in zip(hits[0, :3], fused[0, :3])}
    assert by_doc == {5: (1, 4, 1.0, 6), 6: (3, 1, 3.0, 9), 8: (5, 0, 5.0, 0)}
    assert hits["doc"][0, :3].tolist() == [6, 5, 8]                      # 1/4 + 1/2, 1/2 + 1/5, 1/6


# ---- the row of a given doc against the oracle's ranking ---------------------------------------------------------------------------

@pytest.mark.parametrize("with_prior", [False, True])
def test_score_docs_equals_the_oracle_for_every_ranked_doc(with_prior):
    z = np.load(GOLDEN)
    n_docs = int(z["n_docs"])
    rng = np.random.default_rng(3)
    prior = rng.random((n_docs, 3)) if with_prior else None
    world = {"n_docs": n_docs, "title": (z["t_ptr"], z["t_doc"], z["t_w"]), "body": (z["b_ptr"], z["b_doc"], z["b_w"]),
             "mt": z["t_mag"], "mb": z["b_mag"], "prior": prior}
    n_terms = len(z["b_ptr"]) - 1
    queries = [[0], [1, 2, 3], [4, 4, 9], [hm.UNKNOWN, 5], [n_terms, 6, n_terms + 3], [], list(range(10, 30))]
    for qi, tokens in enumerate(queries):
        probs = rng.random(3) if with_prior else None
        qlen = len(tokens) + (qi % 2)
        docs, T, B, sqd, final = oracle_np.score_topk(n_docs, world["title"], world["body"], world["mt"], world["mb"],
                                                      np.array(tokens, np.uint32), n_docs, query_len=qlen, prior=prior, topic_probs=probs)
        assert (len(docs) > 0) == any(t < n_terms for t in tokens)
        all_docs = np.arange(n_docs, dtype=np.uint32)[None, :]
        out = hm.score_docs(world, np.array([0, len(tokens)], np.uint32), np.array(tokens, np.uint32), all_docs, np.array([n_docs], np.int32),
                            np.zeros((1, n_docs), hm.HIT_DTYPE), query_len=np.array([qlen], np.int32),
                            topic_probs=None if probs is None else probs[None, :])
        rows = out[0, docs.astype(np.int64)]
        for name, ref in (("title", T), ("body", B), ("pagerank", sqd), ("final", final)):
            assert rows[name].tobytes() == np.asarray(ref, np.float64).tobytes(), (qi, name)
        rest = np.setdiff1d(np.arange(n_docs), docs)
        assert (out["title"][0, rest] == 0).all() and (out["body"][0, rest] == 0).all()
        assert (out["final"][0, rest] == (0.33 * out["pagerank"][0, rest]) * 100).all()
        if with_prior and len(rest):
            assert (out["pagerank"][0, rest] > 0).any()
    outside = hm.score_docs(world, np.array([0, 1], np.uint32), np.array([0], np.uint32), np.array([[n_docs, 7]], np.uint32),
                            np.array([1], np.int32), np.full((1, 2), 7, hm.HIT_DTYPE).copy())
    assert outside[0, 0].tobytes() == struct.pack("<II4d", n_docs, 0, 0, 0, 0, 0) and outside[0, 1]["doc"] == 7     # past n_in: untouched


# ---- the ABI and the binding ---------------------------------------------------------------------------------------------------------

def test_layouts_through_the_c_compiler(tmp_path):
    src = tmp_path / "fuse_sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "spaghetti_rank.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d %d\\n", sizeof(ss_fuse_params), offsetof(ss_fuse_params, rrf_c), '
                   'offsetof(ss_fuse_params, w_lex), offsetof(ss_fuse_params, w_vec), sizeof(ss_fused), offsetof(ss_fused, vec_score), '
                   'offsetof(ss_fused, lex_rank), offsetof(ss_fused, vec_rank), SS_FUSE_RRF, SS_FUSE_WEIGHTED, SS_ABI_VERSION); return 0; }\n')
    exe = tmp_path / "fuse_sizes"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert out == ["24", "4", "8", "16", "16", "8", "12", "14", "0", "1", "4"]


def test_binding_declares_the_three_symbols():
    import ctypes
    from spaghettisearch_amd import _lib, engine
    assert len(_lib.PROTOTYPES["ss_score_docs"][1]) == 10 and len(_lib.PROTOTYPES["ss_fuse_hits"][1]) == 20
    assert len(_lib.PROTOTYPES["ss_hybrid_topk"][1]) == 16
    assert ctypes.sizeof(_lib.SsFuseParams) == 24 and ctypes.sizeof(_lib.SsFused) == 16
    assert engine.FUSED_DTYPE == hm.FUSED_DTYPE and engine.FUSED_DTYPE.itemsize == 16
    assert (engine.FUSE_RRF, engine.FUSE_WEIGHTED) == (_lib.SS_FUSE_RRF, _lib.SS_FUSE_WEIGHTED) == (hm.FUSE_RRF, hm.FUSE_WEIGHTED)
    for name in ("score_docs", "fuse_hits", "hybrid_topk"):
        assert callable(getattr(engine.Scorer, name))
    lib = _lib.load()                                             # (loading needs no device)
    for name in ("ss_score_docs", "ss_fuse_hits", "ss_hybrid_topk"):
        assert getattr(lib, name).argtypes == _lib.PROTOTYPES[name][1]


# ---- hybrid_plan.hpp on the host -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("hybrid_plan") / "hybrid_plan_harness")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "hybrid_plan_harness.cpp"), "-o", exe], check=True)
    return exe


def hexd(x):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", x))[0]


def test_plan_harness_scores_and_keys(harness):
    rng = np.random.default_rng(17)
    cases = []
    specials = [0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 1e300, -1e300, 5e-324, -5e-324, 0.1, 100.0]
    for fin in specials:                                          # weighted, the final alone and blended
        cases.append((1, 60, 1.0, 0.0, 1, 0, fin, 0))
        cases.append((1, 60, 0.0, 1.0, 1, 1, fin, 12345))            # 0 * inf and 0 * NaN: NaN
        cases.append((1, 60, -2.5, 0.001, 3, 2, fin, -(2 ** 24)))
    cases.append((1, 60, 1.0, -0.0, 1, 1, -0.0, 0))                  # -0.0 + -0.0: the one way to a stored -0.0
    for _ in range(40):
        cases.append((1, 60, float(rng.normal()), float(rng.normal()), int(rng.integers(0, 5)), int(rng.integers(0, 5)),
                      float(rng.normal() * 100), int(rng.integers(-2 ** 24, 2 ** 24))))
    for c in (1, 60, 2 ** 31 - 1):
        for lr, vr in ((0, 0), (1, 0), (0, 1), (1, 1), (1024, 1024), (7, 300)):
            for wl, wv in ((1.0, 1.0), (0.0, 1.0), (1.0, 0.0), (-1.0, 0.5), (1e308, 1e308)):
                cases.append((0, c, wl, wv, lr, vr, 123.0, 5))
    text = "".join(f"s {m} {c} {hexd(wl)} {hexd(wv)} {lr} {vr} {hexd(fin)} {vs}\n" for m, c, wl, wv, lr, vr, fin, vs in cases)
    r = subprocess.run([harness], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == f"ok {len(cases)} lines"
    keys = []
    for (m, c, wl, wv, lr, vr, fin, vs), line in zip(cases, lines):
        want = hm.fuse_score((m, c, wl, wv), lr, vr, fin, vs)
        bits, key = line.split()
        assert bits == ("7ff8000000000000" if np.isnan(want) else hexd(float(want))), (m, c, wl, wv, lr, vr, fin, vs)
        keys.append((int(key, 16), float(want)))
    assert any(np.isnan(s) for _, s in keys) and any(s == 0 and np.signbit(s) for _, s in keys)
    # ascending keys = the model's order (doc plays no part here: equal keys are ties)
    by_key = sorted(range(len(keys)), key=lambda i: keys[i][0])
    model = sorted(range(len(keys)), key=lambda i: (1, 0.0) if np.isnan(keys[i][1]) else (0, -keys[i][1]))
    assert [keys[i][0] for i in by_key] == [keys[i][0] for i in model]


def test_plan_harness_checks(harness):
    one, inf, nan = hexd(1.0), hexd(np.inf), hexd(np.nan)
    cases = [
        (f"c 1 0 60 {one} {one} 4 100 100 10 0", 0), (f"c 1 1 1 {one} {one} 0 1 1 1 0", 0), (f"c 1 0 60 {one} {one} 4 1024 1024 1024 5000", 0),
        (f"c 0 0 60 {one} {one} 4 100 100 10 0", 1), (f"c 1 2 60 {one} {one} 4 100 100 10 0", 1), (f"c 1 -1 60 {one} {one} 4 100 100 10 0", 1),
        (f"c 1 0 0 {one} {one} 4 100 100 10 0", 1), (f"c 1 0 -5 {one} {one} 4 100 100 10 0", 1), (f"c 1 0 60 {inf} {one} 4 100 100 10 0", 1),
        (f"c 1 0 60 {one} {nan} 4 100 100 10 0", 1), (f"c 1 0 60 {one} {one} -1 100 100 10 0", 1), (f"c 1 0 60 {one} {one} 4 0 100 10 0", 1),
        (f"c 1 0 60 {one} {one} 4 100 0 10 0", 1), (f"c 1 0 60 {one} {one} 4 100 100 0 0", 1), (f"c 1 0 60 {one} {one} 4 100 100 10 -1", 1),
        (f"c 1 0 60 {one} {one} 4 1025 100 10 0", 2), (f"c 1 0 60 {one} {one} 4 100 1025 10 0", 2), (f"c 1 0 60 {one} {one} 4 100 100 1025 0", 2),
        (f"c 1 0 60 {one} {one} 4 0 1025 10 0", 1),                  # an invalid argument is named before an unsupported one
    ]
    r = subprocess.run([harness], input="".join(c + "\n" for c, _ in cases), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split()[:len(cases)] == [str(code) for _, code in cases]
