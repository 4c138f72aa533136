"""CPU checks of ss_facet_counts' definition (tests/facet_model.py): the header's hand-worked known answer, the set model against a
plain per-doc loop on random small tables, and facet_plan.hpp driven on the host under ASan + UBSan (tests/facet_plan_harness.cpp):
elementary intervals, block and word arithmetic, every refusal of the call's own arguments with its code."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import facet_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spaghettisearch_amd", "csrc")
UNKNOWN = 0xFFFFFFFF
I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1
BLOCK = 32768                    # docs of one k_facet_counts workgroup: BLOCK_DOCS in csrc/facet_plan.hpp
OK, INVALID, UNSUPPORTED, STATE = 0, 1, 2, 3


def csr(n_terms, lists):
    """{term: docs} -> (ptr uint64 [n_terms + 1], doc uint32), every list ascending"""
    ptr = np.zeros(n_terms + 1, dtype=np.uint64)
    docs = []
    for t in range(n_terms):
        docs += sorted(lists.get(t, []))
        ptr[t + 1] = len(docs)
    return ptr, np.array(docs, dtype=np.uint32)


# ---- the known answer of the header ---------------------------------------------------------------------------------------------------

def header_world():
    n_docs = 8
    title = csr(3, {0: [1], 2: [6]})
    body = csr(3, {0: [1, 2, 5], 1: [2, 3]})
    fields = np.arange(10, 90, 10, dtype=np.int64)[None, :]
    masks = np.zeros((2, n_docs), dtype=bool)
    masks[0, [0, 1, 2, 3]] = True
    masks[1, [2, 5, 6]] = True
    buckets = [(0, 20, 30), (0, 0, 100), (0, 30, 60), (0, 5, 4)]
    q_ptr, q_terms = np.array([0, 4], np.uint32), np.array([0, 1, 0, UNKNOWN], np.uint32)
    return n_docs, title, body, fields, masks, buckets, q_ptr, q_terms


def test_header_known_answer():
    n_docs, title, body, fields, masks, buckets, q_ptr, q_terms = header_world()
    one = np.array([0, 1], np.uint32)
    cases = [
        ({}, [1, 2, 3, 5], 4, [3, 2], [2, 4, 3, 0]),
        ({"req": (one, np.array([1], np.uint32))}, [2, 3], 2, [2, 1], [1, 2, 2, 0]),
        ({"mask_id": np.array([1], np.int32), "ranges": (one, [(0, 25, 65)])}, [2, 5], 2, [1, 2], [1, 2, 2, 0]),
    ]
    for kw, docs, total, by_mask, by_bucket in cases:
        n_match, mc, bc, sets = fm.facet_counts(n_docs, title, body, q_ptr, q_terms, masks=masks, fields=fields, buckets=buckets, **kw)
        assert np.nonzero(sets[0])[0].tolist() == docs, kw
        assert (int(n_match[0]), mc[0].tolist(), bc[0].tolist()) == (total, by_mask, by_bucket), kw


# ---- the model against a per-doc loop -------------------------------------------------------------------------------------------------

def loop_counts(n_docs, title, body, q_ptr, q_terms, masks, fields, mask_id, req, exc, ranges, buckets):
    def has(table, t, d):
        ptr, doc = table
        return t < len(ptr) - 1 and any(int(doc[j]) == d for j in range(int(ptr[t]), int(ptr[t + 1])))

    def contains(t, d):
        return has(title, t, d) or has(body, t, d)

    n_q = len(q_ptr) - 1
    out = (np.zeros(n_q, np.uint32), np.zeros((n_q, len(masks)), np.uint32), np.zeros((n_q, len(buckets)), np.uint32))
    for q in range(n_q):
        for d in range(n_docs):
            ok = any(contains(int(t), d) for t in q_terms[q_ptr[q]:q_ptr[q + 1]])
            ok = ok and (mask_id[q] < 0 or masks[mask_id[q]][d])
            ok = ok and all(contains(int(t), d) for t in req[1][req[0][q]:req[0][q + 1]])
            ok = ok and not any(contains(int(t), d) for t in exc[1][exc[0][q]:exc[0][q + 1]])
            ok = ok and all(lo <= int(fields[f][d]) <= hi for f, lo, hi in ranges[1][ranges[0][q]:ranges[0][q + 1]])
            if not ok:
                continue
            out[0][q] += 1
            for m in range(len(masks)):
                out[1][q, m] += bool(masks[m][d])
            for b, (f, lo, hi) in enumerate(buckets):
                out[2][q, b] += lo <= int(fields[f][d]) <= hi
    return out


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_model_against_doc_loop(seed):
    rng = np.random.default_rng(seed)
    n_docs, n_terms, n_q = 70, 12, 10
    title = csr(n_terms, {t: rng.choice(n_docs, rng.integers(0, 6), replace=False).tolist() for t in range(n_terms)})
    body = csr(n_terms, {t: rng.choice(n_docs, rng.integers(0, 30), replace=False).tolist() for t in range(n_terms)})
    masks = rng.random((3, n_docs)) < 0.5
    edge = np.array([I64_MIN, -1, 0, 1, I64_MAX], np.int64)
    fields = np.stack([rng.integers(0, 100, n_docs), edge[rng.integers(0, len(edge), n_docs)]]).astype(np.int64)

    def pairs(lo, hi, what):
        lens = rng.integers(lo, hi, n_q)
        ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
        return ptr, [what() for _ in range(int(ptr[-1]))]

    term = lambda: int(rng.integers(0, n_terms + 2))                                                          # noqa: E731
    clause = lambda: (0, int(rng.integers(0, 60)), int(rng.integers(30, 100))) if rng.random() < 0.7 else (1, -1, I64_MAX)   # noqa: E731
    q_ptr, q_terms = pairs(0, 5, term)
    req, exc, ranges = pairs(0, 2, term), pairs(0, 2, term), pairs(0, 3, clause)
    mask_id = rng.integers(-1, 3, n_q).astype(np.int32)
    buckets = [(0, 0, 49), (0, 25, 74), (0, 25, 74), (0, 60, 10), (1, I64_MIN, I64_MIN), (1, I64_MIN, I64_MAX), (1, 0, I64_MAX), (0, 10, 10)]
    q_terms = np.array(q_terms, np.uint32)
    got = fm.facet_counts(n_docs, title, body, q_ptr, q_terms, masks=masks, fields=fields, mask_id=mask_id,
                          req=(req[0], np.array(req[1], np.uint32)), exc=(exc[0], np.array(exc[1], np.uint32)), ranges=ranges, buckets=buckets)
    want = loop_counts(n_docs, title, body, q_ptr, q_terms, masks, fields, mask_id, req, exc, ranges, buckets)
    for g, w in zip(got[:3], want):
        assert g.tolist() == w.tolist()
    assert got[0].sum() > 0 and got[2].sum() > 0


# ---- facet_plan.hpp under the sanitizers ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("facet_plan") / "facet_plan_harness")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "facet_plan_harness.cpp"), "-o", exe], check=True)
    return exe


def ask(harness, lines):
    r = subprocess.run([harness], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert out[-1] == f"ok {len(lines)} lines"
    return out[:-1]


def test_plan_harness_geometry(harness):
    sizes = [1, 31, 32, 33, BLOCK - 1, BLOCK, BLOCK + 1, BLOCK + 37, 2 * BLOCK, 10_000_000, 2 ** 32 - 1]
    out = ask(harness, [f"g {n}" for n in sizes])
    for n, line in zip(sizes, out):
        f = line.split()
        words, blocks = -(-n // 32), -(-n // BLOCK)
        last_words = words - (blocks - 1) * 1024
        last_mask = (1 << (n - (words - 1) * 32)) - 1 if n % 32 else 0xFFFFFFFF
        assert [int(f[0]), int(f[1]), int(f[2]), int(f[3], 16), int(f[4])] == [words, blocks, last_words, last_mask, words], (n, line)
        assert (int(f[5]), int(f[6], 16)) == (0, 0), (n, line)        # nothing past the last block, no valid bit past the last word
    assert ask(harness, ["g 0"])[0].split() == ["0", "0", "0", "00000000", "0", "0", "00000000"]


def test_plan_harness_launches(harness):
    cases = [(0, 5), (5, 0), (1, 1), (306, 1024), (131072, 1024), (131072, 2 ** 31 - 1), (3, 2 ** 30), (131072, 70000)]
    out = ask(harness, [f"l {b} {a}" for b, a in cases])
    for (n_blocks, n_active), line in zip(cases, out):
        f = line.split()
        if n_blocks == 0 or n_active == 0:
            assert f[:2] == ["0", "1"], line
            continue
        per = max(1, (2 ** 31 - 1) // n_active)
        assert int(f[0]) == -(-n_blocks // per) and f[1] == "1" and int(f[2]) <= 2 ** 31 - 1, (n_blocks, n_active, line)
    assert ask(harness, ["l 306 1024"])[0].split() == ["1", "1", str(306 * 1024), "0:306"]


def test_plan_harness_refusals(harness):
    #        n_q q_ptr n_match n_b buckets b_out n_fields
    cases = [((4, 1, 1, 0, 0, 0, 0), OK), ((4, 1, 1, 2, 1, 1, 1), OK), ((0, 0, 0, 0, 0, 0, 0), OK), ((0, 0, 0, 3, 0, 0, 0), OK),
             ((4, 1, 1, 64, 1, 1, 4), OK), ((4, 1, 1, 0, 0, 1, 0), OK),
             ((-1, 1, 1, 0, 0, 0, 0), INVALID), ((4, 1, 0, 0, 0, 0, 0), INVALID), ((4, 0, 1, 0, 0, 0, 0), INVALID),
             ((4, 1, 1, -1, 1, 1, 1), INVALID), ((4, 1, 1, 2, 0, 1, 1), INVALID), ((4, 1, 1, 2, 1, 0, 1), INVALID),
             ((4, 1, 1, 65, 1, 1, 1), UNSUPPORTED), ((0, 1, 1, 65, 1, 1, 1), UNSUPPORTED), ((4, 1, 1, 2 ** 31 - 1, 1, 1, 1), UNSUPPORTED),
             ((4, 1, 1, 1, 1, 1, 0), STATE)]
    out = ask(harness, [" ".join(["a"] + [str(x) for x in c]) for c, _ in cases])
    assert out == [str(code) for _, code in cases]
    fields = [((2, [0, 1, 1, 0]), OK), ((2, []), OK), ((2, [0, 2]), INVALID), ((2, [-1]), INVALID), ((4, [3]), OK), ((1, [1]), INVALID),
              ((1, [2 ** 31 - 1]), INVALID), ((1, [-2 ** 31]), INVALID)]
    out = ask(harness, [" ".join(["f", str(nf), str(len(fs))] + [str(x) for x in fs]) for (nf, fs), _ in fields])
    assert out == [str(code) for _, code in fields]


def bucket_line(buckets, values):
    return " ".join(["b", str(len(buckets))] + [f"{f} {lo} {hi}" for f, lo, hi in buckets] + [str(len(values))] + [f"{f} {v}" for f, v in values])


def check_buckets(harness, buckets, values):
    line = ask(harness, [bucket_line(buckets, values)])[0]
    head, spans, placed = line.split("|")
    n_cuts, field_mask = int(head.split()[0]), int(head.split()[1], 16)
    assert n_cuts <= 2 * len(buckets)
    assert field_mask == sum({1 << f for f, lo, hi in buckets if lo <= hi})
    for (f, lo, hi), span in zip(buckets, spans.split()):
        a, b = (int(x) for x in span.split(":"))
        assert (a < b) == (lo <= hi), (f, lo, hi, span)
    for (f, v), p in zip(values, placed.split()):
        want = sum(1 << k for k, (bf, lo, hi) in enumerate(buckets) if bf == f and lo <= v <= hi)
        assert int(p.split(":")[1], 16) == want, (f, v, p)
    return n_cuts


def test_plan_harness_elementary_intervals(harness):
    probe = [I64_MIN, I64_MIN + 1, -1, 0, 1, 9, 10, 11, 19, 20, 21, 29, 30, 31, 99, 100, 101, I64_MAX - 1, I64_MAX]
    on = lambda f: [(f, v) for v in probe]                                                                     # noqa: E731
    # nested ("past day" inside "past week" inside "past year"), overlapping, repeated, empty, a single value
    assert check_buckets(harness, [(0, 20, 30), (0, 10, 30), (0, 0, 30)], on(0)) == 4
    assert check_buckets(harness, [(0, 0, 20), (0, 10, 30), (0, 10, 30), (0, 30, 10), (0, 20, 20)], on(0)) == 5
    assert check_buckets(harness, [(0, 5, 4)], on(0)) == 0
    assert check_buckets(harness, [], on(0)) == 0
    # the extremes: no cut behind INT64_MAX, a cut at INT64_MIN, the whole axis, one value at either end
    assert check_buckets(harness, [(0, I64_MIN, I64_MAX)], on(0)) == 1
    assert check_buckets(harness, [(0, I64_MIN, I64_MIN), (0, I64_MAX, I64_MAX), (0, I64_MAX, I64_MIN), (0, I64_MIN, -1), (0, 0, I64_MAX)], on(0)) == 4
    assert check_buckets(harness, [(0, I64_MAX - 1, I64_MAX - 1), (0, I64_MIN + 1, I64_MAX - 1)], on(0)) == 3
    # several fields: a value is placed among its own field's cuts only
    assert check_buckets(harness, [(1, 0, 10), (3, 10, 20), (1, 5, 100), (0, 20, 29)], on(0) + on(1) + on(2) + on(3)) == 8
    # SS_MAX_FACET_BUCKETS distinct buckets: the most cuts there can be
    full = [(b % 4, 10 * b, 10 * b + 5) for b in range(64)]
    rng = np.random.default_rng(9)
    vals = [(int(f), int(v)) for f, v in zip(rng.integers(0, 4, 300), rng.integers(-5, 650, 300))]
    assert check_buckets(harness, full, vals) == 128
    # random buckets with random small bounds: overlaps and repeats of every kind
    for seed in range(5):
        rng = np.random.default_rng(seed)
        bk = [(int(rng.integers(0, 2)), int(rng.integers(0, 12)), int(rng.integers(0, 12))) for _ in range(int(rng.integers(1, 65)))]
        check_buckets(harness, bk, [(f, v) for f in (0, 1) for v in range(-1, 14)])
