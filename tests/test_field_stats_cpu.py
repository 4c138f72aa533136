"""CPU checks of ss_field_stats' and ss_field_histogram's definitions (tests/field_stats_model.py): the header's hand-worked known answers,
the model against a plain per-doc Python loop on random small tables, field_stats_plan.hpp driven on the host under ASan + UBSan
(tests/field_stats_plan_harness.cpp): the divider against `/` at the ends of both ranges and on seeded random pairs, the saturated span,
the bin of a value at the ends of the bins and of int64, the edge search at every edge +- 1, the choice of the counting path, the row
stride, the groups under a scratch bound and every refusal of the calls' own arguments with its code; then the header itself: prototypes,
the sizes of the two structs from a compiled C snippet, the ABI version, and the refusals that need no device."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from spaghettisearch_amd import _lib
from tests import field_stats_model as sm
from tests.test_facet_cpu import csr, header_world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spaghettisearch_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "spaghetti_rank.h")
OK, INVALID, UNSUPPORTED, STATE = 0, 1, 2, 3
I64_MIN, I64_MAX, U64_MAX = sm.I64_MIN, sm.I64_MAX, 2 ** 64 - 1
NO_VALUE = sm.NO_VALUE
MAX_BINS = sm.MAX_HIST_BINS


# ---- the known answers of the header ----------------------------------------------------------------------------------------------------

def test_header_known_answers_stats():
    n_docs, title, body, fields, masks, _, q_ptr, q_terms = header_world()
    second = np.array([0, I64_MAX, I64_MAX, I64_MAX, 0, NO_VALUE, 0, 0], np.int64)
    fields = np.stack([fields[0], second])
    one = np.array([0, 1], np.uint32)
    cases = [
        #  arguments                                                          M          count missing min max sum
        (dict(), [1, 2, 3, 5], (4, 0, 20, 60, 150)),
        (dict(req=(one, np.array([1], np.uint32))), [2, 3], (2, 0, 30, 40, 70)),
        (dict(mask_id=np.array([1], np.int32), ranges=(one, [(0, 25, 65)])), [2, 5], (2, 0, 30, 60, 90)),
    ]
    for kw, docs, (count, missing, lo, hi, total) in cases:
        stats, n_match, sets = sm.field_stats(n_docs, title, body, q_ptr, q_terms, fields, [0], masks=masks, **kw)
        assert np.nonzero(sets[0])[0].tolist() == docs and n_match.tolist() == [len(docs)]
        assert stats[0, 0].tolist() == (lo, hi, total, 0, count, missing), kw
    stats, n_match, _ = sm.field_stats(n_docs, title, body, q_ptr, q_terms, fields, [1, 0, 1], masks=masks)
    assert stats[0, 0].tolist() == (I64_MAX, I64_MAX, 0x7FFFFFFFFFFFFFFD, 1, 3, 1) and stats[0, 2].tolist() == stats[0, 0].tolist()
    assert stats[0, 1].tolist() == (20, 60, 150, 0, 4, 0)
    assert sm.stat_of([-1, -1]) == (-1, -1, 0xFFFFFFFFFFFFFFFE, -1, 2, 0)
    assert sm.stat_of([]) == (I64_MAX, I64_MIN, 0, 0, 0, 0) and sm.stat_of([NO_VALUE, NO_VALUE]) == (I64_MAX, I64_MIN, 0, 0, 0, 2)
    empty, n_match, _ = sm.field_stats(n_docs, title, body, np.array([0, 1, 1], np.uint32), np.array([0xFFFFFFFF], np.uint32), fields, [0])
    assert n_match.tolist() == [0, 0] and empty[:, 0].tolist() == [(I64_MAX, I64_MIN, 0, 0, 0, 0)] * 2


def test_header_known_answers_histogram():
    n_docs, title, body, fields, masks, _, q_ptr, q_terms = header_world()
    cases = [
        (dict(origin=15, width=20), [2, 1], 0, 1),
        (dict(origin=35, width=20), [1, 1], 2, 0),
        (dict(edges=[20, 40, 61]), [2, 2], 0, 0),
        (dict(edges=[25, 30, 31]), [0, 1], 1, 2),
    ]
    for kw, counts, below, above in cases:
        got, tails, _ = sm.field_histogram(n_docs, title, body, q_ptr, q_terms, fields, 0, 2, masks=masks, **kw)
        assert got[0].tolist() == counts and tails[0].tolist() == (below, above, 0, 4), kw
    # SS_NO_FIELD_VALUE is missing, not bin 0, even with origin == INT64_MIN
    counts, below, above, missing = sm.histogram_of([NO_VALUE, I64_MIN + 1, I64_MAX, NO_VALUE], 1, origin=I64_MIN, width=1)
    assert (counts.tolist(), below, above, missing) == ([0], 0, 2, 2)
    counts, below, above, missing = sm.histogram_of([NO_VALUE, I64_MIN + 1, I64_MAX], 2, edges=[I64_MIN, 0, I64_MAX])
    assert (counts.tolist(), below, above, missing) == ([1, 0], 0, 1, 1)


# ---- the model against a per-doc loop ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [1, 2, 3])
def test_model_against_doc_loop(seed):
    rng = np.random.default_rng(seed)
    n_docs, n_terms, n_q = 90, 12, 10
    title = csr(n_terms, {t: rng.choice(n_docs, rng.integers(0, 6), replace=False).tolist() for t in range(n_terms)})
    body = csr(n_terms, {t: rng.choice(n_docs, rng.integers(0, 40), replace=False).tolist() for t in range(n_terms)})
    masks = rng.random((3, n_docs)) < 0.7
    pool = np.array([NO_VALUE, I64_MIN + 1, -7, -1, 0, 1, 5, 6, 40, I64_MAX - 1, I64_MAX], np.int64)
    fields = np.stack([rng.integers(0, 8, n_docs), pool[rng.integers(0, len(pool), n_docs)]]).astype(np.int64)
    lens = rng.integers(0, 5, n_q)
    q_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    q_terms = rng.integers(0, n_terms + 2, int(q_ptr[-1])).astype(np.uint32)
    mask_id = rng.integers(-1, 3, n_q).astype(np.int32)
    kw = dict(masks=masks, mask_id=mask_id)
    stats, n_match, sets = sm.field_stats(n_docs, title, body, q_ptr, q_terms, fields, [1, 0], **kw)
    hists = [(dict(origin=-7, width=3), 5), (dict(origin=I64_MIN + 1, width=2 ** 63), 2), (dict(origin=0, width=U64_MAX), 1),
             (dict(edges=[-7, 0, 1, 41, I64_MAX]), 4)]
    got = [sm.field_histogram(n_docs, title, body, q_ptr, q_terms, fields, 1, nb, **h, **kw) for h, nb in hists]
    carried = 0
    for q in range(n_q):
        docs = [d for d in range(n_docs) if sets[q][d]]
        assert len(docs) == n_match[q]
        for i, f in enumerate((1, 0)):
            have = [int(fields[f][d]) for d in docs if int(fields[f][d]) != NO_VALUE]
            s = stats[q, i]
            assert int(s["count"]) == len(have) and int(s["missing"]) == len(docs) - len(have)
            assert int(s["sum_hi"]) * 2 ** 64 + int(s["sum_lo"]) == sum(have)
            assert (int(s["min"]), int(s["max"])) == ((min(have), max(have)) if have else (I64_MAX, I64_MIN))
            carried += int(s["sum_hi"]) != 0
        for (h, nb), (counts, tails, _) in zip(hists, got):
            exp, below, above, missing = [0] * nb, 0, 0, 0
            for d in docs:
                v = int(fields[1][d])
                if v == NO_VALUE:
                    missing += 1
                elif "edges" in h:
                    e = h["edges"]
                    hit = [b for b in range(nb) if e[b] <= v < e[b + 1]]
                    if hit:
                        exp[hit[0]] += 1
                    elif v < e[0]:
                        below += 1
                    else:
                        above += 1
                elif v < h["origin"]:
                    below += 1
                elif (v - h["origin"]) // h["width"] >= nb:
                    above += 1
                else:
                    exp[(v - h["origin"]) // h["width"]] += 1
            assert counts[q].tolist() == exp and tails[q].tolist() == (below, above, missing, len(docs)), (q, h)
            assert sum(exp) + below + above + missing == len(docs)
    assert carried >= 2                                                         # the condition on the inputs: some sum leaves 64 bits


# ---- field_stats_plan.hpp under the sanitizers ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("field_stats_plan") / "field_stats_plan_harness")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "field_stats_plan_harness.cpp"), "-o", exe], check=True)
    return exe


def ask(harness, lines):
    r = subprocess.run([harness], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert out[-1] == f"ok {len(lines)} lines"
    return out[:-1]


WIDTHS = [1, 2, 3, 5, 7, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 63, 2 ** 63 + 1, U64_MAX]


def test_plan_harness_divider(harness):
    """the divider equals `/` for u at 0, 1, around the width, around 2^32 and 2^63 and at 2^64 - 1, for widths at the same places, in the
    form the kernel compiles in for the width; and on seeded random pairs of every magnitude"""
    pairs = []
    for w in WIDTHS + [6, 10, 30, 86400, 2629746, 10 ** 18, U64_MAX - 1]:
        for u in {0, 1, w - 1, w, min(w + 1, U64_MAX), 2 ** 32 - 1, 2 ** 32 + 1, 2 ** 63 - 1, 2 ** 63 + 1, U64_MAX, U64_MAX - w + 1, U64_MAX // w * w,
                  max(U64_MAX // w * w - 1, 0)}:
            pairs.append((u, w))
    out = ask(harness, [f"d {u} {w}" for u, w in pairs])
    kinds = set()
    for (u, w), line in zip(pairs, out):
        q_any, q_kind, q_plain, kind = (int(x) for x in line.split())
        assert q_any == q_kind == q_plain == u // w, (u, w, line)
        assert kind == (1 if w & (w - 1) == 0 else 2)                           # a power of two is a shift
        kinds.add(kind)
    assert kinds == {1, 2}
    assert ask(harness, [f"R {seed} 200000" for seed in (1, 2, 3)]) == ["0", "0", "0"]


def test_plan_harness_span_and_fixed_bins(harness):
    spans = [(0, 1, 1), (0, 30, 6558), (0, 2 ** 63, 2), (0, 2 ** 63, 1), (0, 2 ** 48, 65536), (0, 2 ** 48 - 1, 65536), (0, U64_MAX, 1),
             (0, U64_MAX, 2), (0, 2 ** 63 + 1, 2), (I64_MIN, 2 ** 32 + 1, 65536), (0, (U64_MAX) // 65535, 65535), (0, U64_MAX // 65535 + 1, 65535)]
    out = ask(harness, [f"n {o} {w} {n}" for o, w, n in spans])
    for (o, w, n), line in zip(spans, out):
        span, sat = (int(x) for x in line.split())
        assert sat == int(n * w >= 2 ** 64) and span == min(n * w, U64_MAX), (o, w, n, line)   # saturated at 2^64 - 1, never wrapped
    assert [l.split()[1] for l in out[2:6]] == ["1", "0", "1", "0"] and out[10] == f"{U64_MAX} 0"   # n * w == 2^64 - 1 exactly: not saturated

    def want(o, w, n, v):
        if v == NO_VALUE:
            return n + 2
        if v < o:
            return n
        return (v - o) // w if (v - o) // w < n else n + 1

    cases = []
    for o in (I64_MIN, I64_MIN + 1, -100000, -1, 0, 15, I64_MAX - 10, I64_MAX):
        for w, n in ((1, 1), (1, 3), (2, 5), (7, 300), (30, 6558), (2 ** 63, 2), (U64_MAX, 1), (U64_MAX, 4), (2 ** 63 + 1, 2), (2 ** 48, 65536),
                     (U64_MAX // 65535, 65535)):
            last = o + n * w                                                    # the upper end of the last bin, as a Python integer
            for v in {o - 1, o, o + 1, o + w - 1, o + w, last - 1, last, last + 1, I64_MIN, I64_MIN + 1, -1, 0, I64_MAX - 1, I64_MAX}:
                if I64_MIN <= v <= I64_MAX:
                    cases.append((o, w, n, v))
    out = ask(harness, [f"b {o} {w} {n} {v}" for o, w, n, v in cases])
    seen = set()
    for (o, w, n, v), line in zip(cases, out):
        slot, plain = (int(x) for x in line.split())
        assert slot == plain == want(o, w, n, v), (o, w, n, v, line)
        seen.add("bin" if slot < n else ("below", "above", "missing")[slot - n])
    assert seen == {"bin", "below", "above", "missing"}
    # the named corners: origin - 1 and origin; both sides of the last bin's upper end; the ends of int64 for origins at both ends
    assert ask(harness, ["b 15 20 2 14", "b 15 20 2 15", "b 15 20 2 54", "b 15 20 2 55", f"b {I64_MIN} 1 1 {I64_MIN}", f"b {I64_MIN} 1 1 {I64_MIN + 1}",
                         f"b {I64_MIN + 1} {2 ** 63} 2 {I64_MIN + 1}", f"b {I64_MIN + 1} {2 ** 63} 2 {I64_MAX}", f"b {I64_MAX} 1 1 {I64_MAX}",
                         f"b {I64_MAX} 1 1 {I64_MAX - 1}", f"b {I64_MIN + 1} {U64_MAX} 1 {I64_MAX}", f"b {I64_MIN + 1} {U64_MAX - 1} 1 {I64_MAX}"]) == \
        ["2 2", "0 0", "1 1", "3 3", "3 3", "2 2", "0 0", "1 1", "0 0", "1 1", "0 0", "2 2"]


def test_plan_harness_edges(harness):
    rng = np.random.default_rng(5)
    lists = [[20, 40, 61], [25, 30, 31], [0, 1], [I64_MIN, 0, I64_MAX], [I64_MIN, I64_MIN + 1], [I64_MAX - 1, I64_MAX], [-5, -4, -3, 0, 7, 8, 1000],
             sorted(set(rng.integers(-10 ** 6, 10 ** 6, 1500).tolist())), sorted(set(rng.integers(I64_MIN, I64_MAX, 3000, dtype=np.int64).tolist()))]
    out = ask(harness, [f"E {len(e) - 1} " + " ".join(str(x) for x in e) for e in lists])
    for e, line in zip(lists, out):
        n = len(e) - 1
        got = line.split()
        assert len(got) == 3 * (n + 1)
        for i, x in enumerate(e):
            for j, v in enumerate((x - 1, x, x + 1)):
                if not I64_MIN <= v <= I64_MAX:
                    assert got[3 * i + j] == "x"
                    continue
                want = n + 2 if v == NO_VALUE else n if v < e[0] else n + 1 if v >= e[n] else max(b for b in range(n) if e[b] <= v)
                assert int(got[3 * i + j]) == want, (e[:5], x, v)
    assert ask(harness, ["e 2 41 20 40 61", "e 2 19 20 40 61", "e 2 61 20 40 61", f"e 2 {NO_VALUE} {I64_MIN} 0 {I64_MAX}"]) == ["1", "2", "3", "4"]
    asc = [([1, 2], 1), ([2, 2], 0), ([3, 2], 0), ([I64_MIN, I64_MAX], 1), ([1, 2, 3, 3], 0), ([1, 2, 3, 4], 1), ([0, 5, 4, 6], 0), ([I64_MAX, I64_MIN], 0)]
    assert ask(harness, [f"c {len(e) - 1} " + " ".join(str(x) for x in e) for e, _ in asc]) == [str(a) for _, a in asc]


def test_plan_harness_path_row_and_groups(harness):
    cases = [(1, 8192), (240, 8192), (4096, 8192), (8192, 8192), (8193, 8192), (65536, 8192), (240, 0), (240, -1), (240, 239), (240, 240),
             (8192, 2 ** 40), (8193, 2 ** 40), (1024, 8192), (1025, 8192)]
    out = ask(harness, [f"p {n} {o}" for n, o in cases])
    for (n, o), line in zip(cases, out):
        use, lds, e_in, e_bytes = (int(x) for x in line.split())
        assert use == int(o > 0 and n <= o and n <= 8192), (n, o, line)          # 0 means never; the histogram holds at most 8192 counters
        assert lds % 16 == 0 and n * 4 <= lds < n * 4 + 16
        assert e_in == int(n + 1 <= 1025) and e_bytes == ((n + 1) * 8 if e_in else 0)
        assert lds * use + e_bytes <= 32768 + 8200                              # beside 6.2 KB of static LDS: inside 64 KB
    sizes = [1, 2, 3, 4, 5, 240, 8192, 32787, 65536]
    out = ask(harness, [f"w {n}" for n in sizes])
    for n, line in zip(sizes, out):
        f = [int(x) for x in line.split()]
        assert f[0] % 4 == 0 and n + 4 <= f[0] < n + 8 and f[1:] == [n, n + 1, n + 2, n + 3], (n, line)
    row = lambda n: (n + 4 + 3) // 4 * 16                                       # noqa: E731  (bytes of a counter row)
    groups = [(0, 1024, 240, 0, 0, row(240)), (0, 1024, 65536, 0, 0, row(65536)), (0, 14, 6558, 0, 1, row(6558)), (0, 14, 3, 0, 3 * row(3), row(3)),
              (0, 0, 5, 0, 0, row(5)), (1, 1024, 64, 4, 0, 64 * 4 * 40), (1, 14, 3, 4, 1, 480), (1, 14, 3, 1, 2 * 120 + 7, 120),
              (1, 5, 1, 1, 10 ** 15, 40), (1, 3000, 131072, 4, 0, 131072 * 160)]
    out = ask(harness, [f"s {k} {a} {x} {y} {opt}" for k, a, x, y, opt, _ in groups])
    for (k, a, x, y, opt, qb), line in zip(groups, out):
        group, n_groups, covered, bytes_ = (int(v) for v in line.split())
        scratch = opt if opt >= 1 else 256 << 20
        assert bytes_ == qb and covered == 1
        assert group == min(a, max(1, scratch // qb)) and n_groups == (-(-a // group) if a else 0), (k, a, x, y, opt, line)
    assert [l.split()[:2] for l in out[:4]] == [["1024", "1"], ["1023", "2"], ["1", "14"], ["3", "5"]]
    assert out[6].split()[:2] == ["1", "14"] and out[7].split()[:2] == ["2", "7"]


def test_plan_harness_refusals(harness):
    #         n_q q_ptr out n_stat_fields has_fields n_fields f0 f1 f2 f3
    stats = [((4, 1, 1, 1, 1, 4, 0, 0, 0, 0), OK), ((4, 1, 1, 4, 1, 4, 3, 2, 1, 0), OK), ((4, 1, 1, 3, 1, 4, 2, 2, 2, 9), OK),
             ((-1, 1, 1, 1, 1, 4, 0, 0, 0, 0), INVALID), ((4, 0, 1, 1, 1, 4, 0, 0, 0, 0), INVALID), ((4, 1, 0, 1, 1, 4, 0, 0, 0, 0), INVALID),
             ((4, 1, 1, 0, 1, 4, 0, 0, 0, 0), INVALID), ((4, 1, 1, -3, 1, 4, 0, 0, 0, 0), INVALID), ((4, 1, 1, 1, 0, 4, 0, 0, 0, 0), INVALID),
             ((4, 1, 1, 5, 1, 4, 0, 0, 0, 0), UNSUPPORTED), ((4, 1, 1, 2 ** 31 - 1, 1, 4, 0, 0, 0, 0), UNSUPPORTED),
             ((4, 1, 1, 1, 1, 0, 0, 0, 0, 0), STATE),
             ((4, 1, 1, 1, 1, 4, 4, 0, 0, 0), INVALID), ((4, 1, 1, 1, 1, 4, -1, 0, 0, 0), INVALID), ((4, 1, 1, 4, 1, 4, 0, 1, 2, 4), INVALID),
             ((4, 1, 1, 2, 1, 1, 0, 1, 0, 0), INVALID),
             # n_q == 0 is SS_OK whatever else is wrong
             ((0, 0, 0, 0, 0, 0, 9, 9, 9, 9), OK), ((0, 0, 0, 99, 0, 4, 0, 0, 0, 0), OK)]
    assert ask(harness, [" ".join(["a"] + [str(x) for x in c]) for c, _ in stats]) == [str(code) for _, code in stats]
    #         n_q q_ptr out field width has_edges n_bins n_fields [edges]
    hist = [((4, 1, 1, 0, 1, 0, 1, 4), OK), ((4, 1, 1, 3, U64_MAX, 0, MAX_BINS, 4), OK), ((4, 1, 1, 0, 0, 1, 2, 4, 1, 2, 3), OK),
            ((4, 1, 1, 0, 0, 1, 1, 4, I64_MIN, I64_MAX), OK),
            ((-1, 1, 1, 0, 1, 0, 1, 4), INVALID), ((4, 0, 1, 0, 1, 0, 1, 4), INVALID), ((4, 1, 0, 0, 1, 0, 1, 4), INVALID),
            ((4, 1, 1, 0, 1, 0, 0, 4), INVALID), ((4, 1, 1, 0, 1, 0, -7, 4), INVALID), ((4, 1, 1, 0, 0, 0, 5, 4), INVALID),
            ((4, 1, 1, 4, 1, 0, 5, 4), INVALID), ((4, 1, 1, -1, 1, 0, 5, 4), INVALID),
            ((4, 1, 1, 0, 0, 1, 2, 4, 1, 2, 2), INVALID), ((4, 1, 1, 0, 0, 1, 2, 4, 1, 3, 2), INVALID), ((4, 1, 1, 0, 7, 1, 1, 4, 5, 5), INVALID),
            ((4, 1, 1, 0, 1, 0, MAX_BINS + 1, 4), UNSUPPORTED), ((4, 1, 1, 0, 1, 1, 2 ** 31 - 1, 4), UNSUPPORTED),
            ((4, 1, 1, 0, 1, 0, 5, 0), STATE),
            ((0, 0, 0, 9, 0, 0, 0, 0), OK), ((0, 0, 0, 0, 0, 1, MAX_BINS + 1, 4), OK)]
    assert ask(harness, [" ".join(["h"] + [str(x) for x in c]) for c, _ in hist]) == [str(code) for _, code in hist]


# ---- the header and the library, without a device ---------------------------------------------------------------------------------------

def test_header_prototypes_struct_sizes_and_abi_version(tmp_path):
    text = open(HEADER).read()
    assert re.search(r"^#define SS_ABI_VERSION 4$", text, re.M) and re.search(r"^#define SS_MAX_HIST_BINS 65536$", text, re.M)
    block = text[:text.index("#define SS_ABI_VERSION")]
    for name in ("SS_MAX_HIST_BINS", "ss_field_stat", "ss_hist_tail", "ss_field_stats", "ss_field_histogram"):
        assert name in block, name                                               # the ABI comment block names what was added under 4
    common = ["s", "n_q", "q_ptr", "q_terms", "mask_id", "req_ptr", "req_terms", "exc_ptr", "exc_terms", "rng_ptr", "rng"]
    names = {}
    for fn, own in (("ss_field_stats", ["n_stat_fields", "fields", "stats_out", "n_match_out"]),
                    ("ss_field_histogram", ["field", "origin", "width", "edges", "n_bins", "counts_out", "tails_out"])):
        proto = re.search(r"int32_t %s\(([^;]*)\);" % fn, text).group(1)
        params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", proto).split(",")]
        assert [p.split()[-1] for p in params] == common + own, fn
        assert len(_lib.PROTOTYPES[fn][1]) == len(params)
        names[fn] = params
    assert names["ss_field_stats"][12] == "const int32_t* fields" and names["ss_field_stats"][13].startswith("ss_field_stat*")
    assert names["ss_field_histogram"][12:15] == ["int64_t origin", "uint64_t width", "const int64_t* edges"]
    assert names["ss_field_histogram"][17].startswith("ss_hist_tail*")
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "spaghetti_rank.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(ss_field_stat), offsetof(ss_field_stat, min), '
                   'offsetof(ss_field_stat, max), offsetof(ss_field_stat, sum_lo), offsetof(ss_field_stat, sum_hi), offsetof(ss_field_stat, count), '
                   'offsetof(ss_field_stat, missing), sizeof(ss_hist_tail), offsetof(ss_hist_tail, above), offsetof(ss_hist_tail, missing), '
                   'offsetof(ss_hist_tail, n_match), SS_ABI_VERSION); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == \
        ["40", "0", "8", "16", "24", "32", "36", "16", "4", "8", "12", "4"]
    from spaghettisearch_amd import engine
    assert engine.FIELD_STAT_DTYPE == sm.FIELD_STAT_DTYPE and engine.HIST_TAIL_DTYPE == sm.HIST_TAIL_DTYPE
    assert sm.FIELD_STAT_DTYPE.itemsize == 40 and sm.HIST_TAIL_DTYPE.itemsize == 16


def test_refusals_without_a_device():
    """a NULL handle is refused before anything looks for a device"""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libspaghetti_rank.so is not built")
    lib = _lib.load()
    assert lib.ss_abi_version() == 4
    buf = (ctypes.c_uint32 * 16)()
    p = ctypes.addressof(buf)
    assert lib.ss_field_stats(None, 1, p, p, None, None, None, None, None, None, None, 1, p, p, p) == INVALID
    assert lib.ss_field_stats(None, 0, None, None, None, None, None, None, None, None, None, 0, None, None, None) == INVALID
    assert lib.ss_field_histogram(None, 1, p, p, None, None, None, None, None, None, None, 0, 0, 1, None, 1, p, p) == INVALID
    assert lib.ss_field_histogram(None, 0, None, None, None, None, None, None, None, None, None, 0, 0, 0, None, 0, None, None) == INVALID
    assert bytes(buf) == bytes(64)
