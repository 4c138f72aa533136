"""CPU checks of the vector-list feature: the header's three prototypes and two macros under an unchanged SS_ABI_VERSION, the ctypes
signatures and engine methods, the numpy model (tests/vector_lists_model.py) against a plain Python loop on a hand-written case of 9
docs and 3 lists (one list empty, one doc at SS_NO_LIST, two centroids with equal scores), and the segment / slot / batch planner
(spaghettisearch_amd/csrc/vector_lists_plan.hpp) through tests/vector_lists_plan_harness.cpp: a stand-alone program compiled with the
host C++ compiler, no device header on the include path, AddressSanitizer + UBSan."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import vector_lists_model as vlm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spaghetti_rank.h")
CSRC = os.path.join(ROOT, "spaghettisearch_amd", "csrc")
VEC_HIT = np.dtype([("doc", "<u4"), ("score", "<i4")])
NAMES = (("ss_scorer_set_vector_lists", 4), ("ss_vector_assign_lists", 5), ("ss_vector_topk_probed", 9))
TILE, PART_BYTES = 64, 256 << 20


def test_header_carries_the_new_entry_points_under_abi_4():
    text = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"#define SS_ABI_VERSION 4\b", code)
    for name, n_params in NAMES:
        m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*?)\)\s*;", code, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == n_params, name
        assert name in text.split("#define SS_ABI_VERSION")[0], name              # listed in the ABI comment block
    assert re.search(r"#define SS_MAX_VEC_LISTS\s+65536\b", code) and re.search(r"#define SS_NO_LIST\s+0xFFFFFFFFu", code)
    assert (vlm.MAX_LISTS, vlm.NO_LIST) == (65536, 0xFFFFFFFF)
    assert "byte for byte" in text.split("ss_scorer_set_vector_lists")[1]         # the identity with ss_vector_topk is stated


def test_lib_carries_the_signatures():
    from spaghettisearch_amd import _lib, engine
    for name, n_params in NAMES:
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == n_params, name
    assert (_lib.SS_MAX_VEC_LISTS, _lib.SS_NO_LIST, engine.NO_LIST) == (65536, 0xFFFFFFFF, 0xFFFFFFFF)
    for method in ("set_vector_lists", "assign_vector_lists", "vector_topk_probed"):
        assert callable(getattr(engine.Scorer, method))
    assert callable(engine.train_vector_lists)


# ---- the model against a plain loop, by hand ---------------------------------------------------------------------------------------
DOCS = [[5, 0, 0], [0, 4, 0], [4, 0, 0], [0, 0, 9], [0, 5, 0], [3, 3, 0], [9, 9, 0], [1, 0, 0], [0, 1, 0]]
LISTS = [0, 1, 0, vlm.NO_LIST, 1, 0, 1, 0, 1]                  # list 2 is empty; doc 3 is in no list
CENTROIDS = [[1, 0, 0], [0, 1, 0], [1, 0, 0]]                  # lists 0 and 2 tie under every query
QUERIES = [[2, 1, 0], [1, 2, 0], [0, 0, 1], [1, 1, 0]]         # query 3 ties all three centroids


def pad64(rows):
    a = np.zeros((len(rows), 64), np.int8)
    a[:, :3] = rows
    return a


def brute(a, b):
    return sum(int(x) * int(y) for x, y in zip(a, b))


def loop_probes(q, n_probe):
    return sorted(range(len(CENTROIDS)), key=lambda l: (-brute(q, CENTROIDS[l]), l))[:n_probe]


def test_model_against_a_loop_on_nine_docs():
    vec, cent, qvec = pad64(DOCS), pad64(CENTROIDS), pad64(QUERIES)
    lod = np.array(LISTS, np.uint32)
    assert vlm.probes(qvec, cent, 1).tolist() == [[0], [1], [0], [0]]
    assert vlm.probes(qvec, cent, 2).tolist() == [[0, 2], [1, 0], [0, 1], [0, 1]]     # the tie of lists 0 and 2 goes to list 0
    assert vlm.probes(qvec, cent, 9).shape == (4, 3)
    for n_probe in (1, 2, 3, 7):
        for k in (1, 3, 9):
            hits, n_hits, pr = vlm.topk_probed(qvec, vec, cent, lod, k, n_probe, np.full((4, k), 77, np.int64).view(VEC_HIT).copy(),
                                               np.full(4, -7, np.int32))
            for q, qv in enumerate(QUERIES):
                pl = loop_probes(qv, n_probe)
                assert pr[q].tolist() == pl
                cands = [d for d in range(9) if LISTS[d] in pl]
                order = sorted(cands, key=lambda d: (-brute(qv, DOCS[d]), d))[:k]
                assert n_hits[q] == len(order)
                assert hits["doc"][q, :len(order)].tolist() == order
                assert hits["score"][q, :len(order)].tolist() == [brute(qv, DOCS[d]) for d in order]
                assert hits[q, len(order):].tobytes() == np.full(k - len(order), 77, np.int64).tobytes()
                assert 3 not in order                                              # the doc in no list, the best one of query 2
    # query 2 probes list 0 and then the empty list 2: only list 0's docs, all at score 0, by doc id
    hits, n_hits, pr = vlm.topk_probed(qvec[2:3], vec, cent, lod, 9, 2, np.zeros((1, 9), VEC_HIT), np.zeros(1, np.int32))
    assert pr.tolist() == [[0, 1]] and n_hits.tolist() == [8]
    cent2 = pad64([[0, 0, 1], [0, 1, 0], [0, 0, 1]])
    hits, n_hits, pr = vlm.topk_probed(qvec[2:3], vec, cent2, lod, 9, 2, np.zeros((1, 9), VEC_HIT), np.zeros(1, np.int32))
    assert pr.tolist() == [[0, 2]] and n_hits.tolist() == [4] and hits["doc"][0, :4].tolist() == [0, 2, 5, 7]
    # an allow-list on top
    masks = np.zeros((1, 9), bool)
    masks[0, [2, 3, 4]] = True
    hits, n_hits, _ = vlm.topk_probed(qvec[:1], vec, cent, lod, 5, 1, np.zeros((1, 5), VEC_HIT), np.zeros(1, np.int32), [0], masks)
    assert n_hits.tolist() == [1] and hits["doc"][0, 0] == 2
    # assign: the largest centroid score, the lower list on a tie (lists 0 and 2 always tie; doc 5 ties all three)
    lists, sc = vlm.assign(vec, cent)
    want = [min(range(3), key=lambda l: (-brute(d, CENTROIDS[l]), l)) for d in DOCS]
    assert lists.tolist() == want == [0, 1, 0, 0, 1, 0, 0, 0, 1] and lists.dtype == np.uint32
    assert sc.tolist() == [max(brute(d, c) for c in CENTROIDS) for d in DOCS] and sc.dtype == np.int32


def test_model_train_keeps_an_empty_lists_centroid():
    rng = np.random.default_rng(3)
    vec = rng.integers(-20, 21, (50, 64)).astype(np.int8)
    c0 = vec[np.sort(np.random.default_rng(1).choice(50, size=6, replace=False))]
    cent, lod = vlm.train(vec, 6, 2, 1)
    assert cent.shape == (6, 64) and cent.dtype == np.int8 and lod.shape == (50,) and lod.dtype == np.uint32
    assert lod.tolist() == vlm.assign(vec, cent)[0].tolist()
    assert vlm.train(vec, 6, 0, 1)[0].tobytes() == c0.tobytes()                    # no iteration: the sample rows
    # two kinds of rows and three lists: two centroids are equal whatever is drawn, the higher one's list is empty and keeps its row
    two = np.where((np.arange(40) % 2 == 0)[:, None], np.full(64, 9, np.int8), np.full(64, -9, np.int8)).astype(np.int8)
    start = two[np.sort(np.random.default_rng(5).choice(40, size=3, replace=False))]
    cent, lod = vlm.train(two, 3, 3, 5)
    empty = [l for l in range(3) if not (lod == l).any()]
    assert empty and all(cent[l].tobytes() == start[l].tobytes() for l in empty)


# ---- the planner ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("vector_lists_plan") / "vector_lists_plan_harness")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "vector_lists_plan_harness.cpp"), "-o", exe], check=True)
    return exe


def run(harness, lines):
    r = subprocess.run([harness], input="".join(line + "\n" for line in lines), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert out[-1] == f"ok {len(lines)} lines"
    return [[int(x) for x in line.split()] for line in out[:-1]]


def plan_line(dim, n_q, k, n_probe, opt_seg, opt_batch, runs, n_cu=256, lds=160 << 10):
    return f"P {dim} {n_q} {k} {n_probe} {opt_seg} {opt_batch} {n_cu} {lds} {len(runs)} " + " ".join(f"{a} {b}" for a, b in runs)


def test_seg_rows_and_assign_batch(harness):
    src = open(os.path.join(CSRC, "vector_lists_plan.hpp")).read()
    assert re.search(r"constexpr uint32_t MAX_LISTS = 65536;", src)
    got = run(harness, ["S 64 1000 7 256", "S 1 1000 7 256", "S 65 1000 7 256", "S 128 0 1 256", "S 0 1000 70 256", "S 0 10000000 4096 256",
                        "S 0 10000000 1 256", "S 0 0 5 0", "S 99999999999 10 1 1", "A 0", "A 100", "A 99999999"])
    assert [g[0] for g in got[:4]] == [64, 64, 128, 128]                              # rounded up to the tile
    assert got[4][0] == 4 * TILE                                                      # a small table: one round of the workgroup
    assert got[5][0] == -(-(10_000_000 // 1024) // TILE) * TILE                       # 4096 even lists of 2441: the spread over 4 x 256 items wins
    assert got[5][0] >= 2 * (10_000_000 // 4096) and got[6][0] == -(-(2 * 10_000_000) // TILE) * TILE
    assert got[7][0] == 4 * TILE and got[8][0] == 1 << 31
    assert [g[0] for g in got[9:]] == [65535 * 16, 100, 65535 * 16]


def test_plan_harness(harness):
    cases = {
        "even": plan_line(128, 1024, 100, 32, 0, 0, [(2441, 4096)]),
        "seg64": plan_line(64, 17, 10, 3, 64, 0, [(900, 1), (0, 1), (1, 1), (63, 1), (64, 1), (65, 1)]),
        "one list": plan_line(128, 1024, 100, 32, 0, 0, [(10_000_000, 1), (0, 4095)]),
        "all empty": plan_line(64, 5, 10, 4, 0, 0, [(0, 7)]),
        "probe above lists": plan_line(64, 5, 10, 1024, 0, 0, [(100, 7)]),
        "limits": plan_line(64, 33, 1024, 1024, 0, 0, [(2, 1500)]),
        "most lists": plan_line(64, 3, 1024, 1024, 0, 0, [(3, 65536)]),
        "forced batch": plan_line(64, 130, 10, 3, 0, 7, [(150, 7)]),
        "one query too many": plan_line(128, 100, 1024, 8, 64, 0, [(1 << 20, 8)]),
        "too large": plan_line(128, 1, 1024, 1024, 64, 0, [(1 << 22, 1024)]),
        "small lds": plan_line(1024, 4, 1024, 4, 0, 0, [(10, 4)], lds=64 << 10),
        "no lists": plan_line(64, 4, 10, 4, 0, 0, []),
    }
    names = list(cases)
    out = dict(zip(names, run(harness, [cases[n] for n in names])))
    for name, row in out.items():
        ok, too_large, n_probe, seg_rows, slots, q_batch, n_batches, part_keys, q_block, cap, lds_bytes, slots_by_def = row
        if name in ("too large", "small lds", "no lists"):
            assert not ok, name
            continue
        assert ok and not too_large, name
        assert seg_rows % TILE == 0 and slots == max(slots_by_def, 1), name        # the bound is the sum of the n_probe largest segment counts
        assert q_block in (16, 32, 64) and lds_bytes <= 160 << 10, name
    ok, _, n_probe, seg_rows, slots, q_batch, n_batches, part_keys, *_ = out["even"]
    assert (n_probe, slots, n_batches, q_batch >= 1024) == (32, 32, 1, True) and part_keys == 1024 * 32 * 100
    # seg_rows 64: 900 -> 15 segments, 65 -> 2, 64 -> 1; the three largest lists are probed in the worst case
    assert out["seg64"][2:5] == [3, 64, 15 + 2 + 1] and out["seg64"][6] == 1
    # one list holding every doc: cut into about 4 x 256 segments, and the call into batches that keep the partial lists at 256 MB
    ok, _, _, seg_rows, slots, q_batch, n_batches, part_keys, *_ = out["one list"]
    assert 1000 <= slots <= 1100 and n_batches == -(-1024 // q_batch) and n_batches > 1
    assert q_batch == PART_BYTES // (slots * 100 * 8) and part_keys * 8 <= PART_BYTES
    assert out["all empty"][2:5] == [4, 4 * TILE, 1] and out["all empty"][7] == 5 * 10   # no segment at all: one slot per query is still planned
    assert out["probe above lists"][2] == 7 and out["probe above lists"][4] == 7
    assert out["limits"][2] == 1024 and out["limits"][4] == 1024 and out["limits"][8] == 16
    assert out["most lists"][2] == 1024 and out["most lists"][4] == 1024
    assert out["forced batch"][5:7] == [7, 19]
    # 8 lists of 2^20 rows at 64 rows per segment: 2^17 slots of 8 KB per query -> one query per batch, still in bound per batch + one query
    ok, _, _, _, slots, q_batch, n_batches, part_keys, *_ = out["one query too many"]
    assert slots == 8 << 14 and q_batch == 1 and n_batches == 100 and part_keys == slots * 1024
    assert out["too large"][1] == 1                                                  # more than 2^31 keys for one query: SS_ERR_OOM, not planned
    assert out["small lds"][1] == 0 and out["no lists"][:2] == [0, 0]
