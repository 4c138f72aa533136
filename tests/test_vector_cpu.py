"""CPU checks of the doc-vector feature: the header's four prototypes and three macros under an unchanged SS_ABI_VERSION,
sizeof(ss_vec_hit) through a compiled C snippet, the ctypes signatures, the numpy model (tests/vector_model.py) against a brute-force
Python loop on a hand-written 7-doc case with ties, and the chunk / query-block planner (spaghettisearch_amd/csrc/vector_plan.hpp)
through tests/vector_plan_harness.cpp: a stand-alone program compiled with the host C++ compiler, no device header on the include
path, AddressSanitizer + UBSan."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import vector_model as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spaghetti_rank.h")
CSRC = os.path.join(ROOT, "spaghettisearch_amd", "csrc")
VEC_HIT = np.dtype([("doc", "<u4"), ("score", "<i4")])
HIT = np.dtype([("doc", "<u4"), ("_pad", "<u4"), ("title", "<f8"), ("body", "<f8"), ("pagerank", "<f8"), ("final", "<f8")])
NAMES = (("ss_scorer_set_doc_vectors", 3), ("ss_vector_topk", 7), ("ss_hit_vector_scores", 7), ("ss_rerank_hits_by_vector", 11))


def test_header_carries_the_new_entry_points_under_abi_4():
    text = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"#define SS_ABI_VERSION 4\b", code)
    for name, n_params in NAMES:
        m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*?)\)\s*;", code, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == n_params, name
        assert name in text.split("#define SS_ABI_VERSION")[0], name              # listed in the ABI comment block
    assert re.search(r"#define SS_MAX_VEC_DIM\s+1024\b", code) and re.search(r"#define SS_NO_VEC_SCORE\s+INT32_MIN\b", code)
    assert re.search(r"typedef struct ss_vec_hit \{ uint32_t doc; int32_t score; \} ss_vec_hit;", code)
    assert (vm.MAX_DIM, vm.NO_SCORE) == (1024, -(2 ** 31))


def test_lib_carries_the_signatures():
    from spaghettisearch_amd import _lib, engine
    for name, n_params in NAMES:
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == n_params, name
    assert (_lib.SS_MAX_VEC_DIM, _lib.SS_NO_VEC_SCORE) == (1024, -(2 ** 31))
    assert ctypes.sizeof(_lib.SsVecHit) == 8 == engine.VEC_HIT_DTYPE.itemsize
    assert [engine.VEC_HIT_DTYPE.fields[n][1] for n in ("doc", "score")] == [0, 4]
    for method in ("set_doc_vectors", "vector_topk", "hit_vector_scores", "rerank_hits_by_vector"):
        assert callable(getattr(engine.Scorer, method))


def test_vec_hit_is_8_bytes(tmp_path):
    src = tmp_path / "vec_hit_size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "spaghetti_rank.h"\n'
                   'int main(void) { printf("%zu %zu %zu %d\\n", sizeof(ss_vec_hit), offsetof(ss_vec_hit, doc), offsetof(ss_vec_hit, score), '
                   'SS_MAX_VEC_DIM); return SS_NO_VEC_SCORE < -(1 << 24) ? 0 : 1; }\n')
    exe = tmp_path / "vec_hit_size"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert out == ["8", "0", "4", "1024"]


# ---- the model against a brute-force loop, by hand --------------------------------------------------------------------------------
#        position 0    1    2   3 ...
DOCS = [[1, 0, 0], [0, 2, 0], [1, 0, 0], [-128, 0, 0], [0, 0, 0], [0, 2, 0], [3, -1, 0]]       # docs 0 / 2 and 1 / 5 are twins; doc 4 is all zero
QUERIES = [[2, 1, 0], [-128, 0, 5], [0, 0, 0]]


def pad64(rows):
    a = np.zeros((len(rows), 64), np.int8)
    a[:, :3] = rows
    return a


def brute(q, d):
    return sum(int(a) * int(b) for a, b in zip(q, d))


def test_model_against_a_loop_on_seven_docs():
    vec, qvec = pad64(DOCS), pad64(QUERIES)
    sc = vm.scores(qvec, vec)
    assert sc.dtype == np.int32 and sc.tolist() == [[brute(q, d) for d in DOCS] for q in QUERIES]
    assert sc.tolist() == [[2, 2, 2, -256, 0, 2, 5], [-128, 0, -128, 16384, 0, 0, -384], [0] * 7]
    for k in (1, 3, 5, 7, 9):
        hits, n_hits = vm.topk(qvec, vec, k, np.full((3, k), 77, VEC_HIT).view(VEC_HIT), np.full(3, -7, np.int32))
        for q in range(3):
            order = sorted(range(7), key=lambda d: (-brute(QUERIES[q], DOCS[d]), d))[:k]
            assert n_hits[q] == len(order) == min(k, 7)
            assert hits["doc"][q, :len(order)].tolist() == order
            assert hits["score"][q, :len(order)].tolist() == [brute(QUERIES[q], DOCS[d]) for d in order]
    hits, _ = vm.topk(qvec, vec, 5, np.zeros((3, 5), VEC_HIT), np.zeros(3, np.int32))
    assert hits["doc"].tolist() == [[6, 0, 1, 2, 5], [3, 1, 4, 5, 0], [0, 1, 2, 3, 4]]              # ties by doc id, a tie across k = 5 in row 0
    # allow-lists: an empty one leaves the row alone, -1 is every doc
    masks = np.zeros((2, 7), bool)
    masks[1, [5, 2, 3]] = True
    hits, n_hits = vm.topk(qvec, vec, 2, np.full((3, 2), 9, np.int64).view(VEC_HIT).copy(), np.zeros(3, np.int32), [0, 1, -1], masks)
    assert n_hits.tolist() == [0, 2, 2] and hits["doc"][1].tolist() == [3, 5] and hits["doc"][2].tolist() == [0, 1]
    assert hits[0].tobytes() == np.full(2, 9, np.int64).tobytes()


def test_model_rerank_is_stable_and_pages():
    vec, qvec = pad64(DOCS), pad64(QUERIES[:1])
    window = np.zeros((1, 8), HIT)
    window["doc"][0] = [5, 3, 7, 0, 6, 2, 0xFFFFFFFF, 1]                          # 7 and 0xFFFFFFFF are outside the table
    window["final"][0] = np.arange(8) + 0.5                                       # marks the window position
    window["_pad"][0] = 0xABCD

    def page(first, k, n=8):
        out = vm.rerank(qvec, vec, window, np.array([n], np.int32), first, k, np.zeros((1, k), HIT), np.full(1, -7, np.int32), np.full((1, k), 99, np.int32))
        cnt = int(out[1][0])
        assert (out[0]["_pad"][0, :cnt] == 0xABCD).all() and (out[2][0, cnt:] == 99).all()
        return [int(x - 0.5) for x in out[0]["final"][0, :cnt]], out[2][0, :cnt].tolist()
    # scores 2 (positions 0, 3, 5, 7 in window order), 5 (position 4), -256 (position 1); outside rows last
    assert page(0, 8) == ([4, 0, 3, 5, 7, 1, 2, 6], [5, 2, 2, 2, 2, -256, vm.NO_SCORE, vm.NO_SCORE])
    assert page(2, 3)[0] == [3, 5, 7] and page(7, 4)[0] == [6] and page(8, 4) == ([], []) and page(9, 1) == ([], [])
    assert page(0, 8, n=3) == ([0, 1, 2], [2, -256, vm.NO_SCORE]) and page(0, 2, n=0) == ([], [])
    got = vm.hit_scores(qvec, vec, window, np.array([7], np.int32), np.full((1, 8), 99, np.int32))
    assert got.tolist() == [[2, -256, vm.NO_SCORE, 2, 5, 2, vm.NO_SCORE, 99]]


# ---- the planner ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("vector_plan") / "vector_plan_harness")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "vector_plan_harness.cpp"), "-o", exe], check=True)
    return exe


def test_plan_harness(harness):
    src = open(os.path.join(CSRC, "vector_plan.hpp")).read()
    tile = int(re.search(r"constexpr uint32_t TILE = (\d+);", src).group(1))
    gpu_test = open(os.path.join(ROOT, "tests", "test_gpu_vector.py")).read()
    assert re.search(r"^TILE = (\d+)", gpu_test, flags=re.M).group(1) == str(tile)
    lds = 160 << 10
    cases = []
    for n_docs in (0, 1, tile - 1, tile, tile + 1, 1000, 4099, 10_000_000):
        for chunk in (0, tile, 1, 3 * tile + 1):                                  # the default, one tile, and sizes rounded up to the tile
            for n_q, k in ((1, 1), (1, 1024), (1025, 10), (17, n_docs + 5 if n_docs + 5 <= 1024 else 1024), (1024, 100)):
                for dim in (64, 128, 1024):
                    cases.append((n_docs, dim, n_q, k, chunk, 256, lds))
    cases += [(1000, 128, 33, 10, 0, 1, lds), (1000, 128, 33, 10, 0, 256, 64 << 10), (4099, 1024, 33, 1024, 0, 256, 64 << 10)]
    text = "".join(" ".join(str(x) for x in case) + "\n" for case in cases)
    r = subprocess.run([harness], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == f"ok {len(cases)} lines"
    many = 0
    for case, line in zip(cases, lines):
        n_docs, dim, n_q, k, chunk, n_cu, lds_limit = case
        ok, too_large, q_block, n_qblocks, chunk_docs, n_chunks, cap, row_stride, lds_bytes, part_keys = (int(x) for x in line.split())
        if lds_limit == lds:
            assert ok == 1 and too_large == 0, case                               # every shape of the ABI fits the device's LDS
        if not ok:
            continue
        assert n_chunks == -(-n_docs // chunk_docs) and n_qblocks == -(-n_q // q_block), case
        if chunk:
            assert chunk_docs == -(-chunk // tile) * tile, case
        many += n_docs == 1000 and chunk == tile and n_chunks == 16
    assert many > 0                                                               # a tile-sized chunk makes many chunks of a few hundred docs
    # 64 KB of LDS cannot hold 16 queries at k = 1024: refused, not planned wrongly
    assert lines[len(cases) - 1].split()[0] == "0"
