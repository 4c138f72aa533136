"""CPU checks of ss_field_topk's definition (tests/field_topk_model.py): the header's hand-worked known answers, the model against a plain
per-doc Python sort on random small tables, and field_topk_plan.hpp driven on the host under ASan + UBSan
(tests/field_topk_plan_harness.cpp): the key transform at the ends of the value range, the runs of a query and their tiling, the
candidate buffer, the groups under a scratch bound, the launch cuts, every refusal of the call's own arguments with its code."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import field_topk_model as tm
from tests.test_facet_cpu import csr, header_world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spaghettisearch_amd", "csrc")
UNKNOWN = 0xFFFFFFFF
I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1
OK, INVALID, UNSUPPORTED, STATE = 0, 1, 2, 3
MAX_TOPK = 1024


# ---- the known answers of the header ----------------------------------------------------------------------------------------------------

def test_header_known_answers():
    n_docs, title, body, fields, masks, _, q_ptr, q_terms = header_world()
    fields = np.concatenate([fields, np.array([[5, 7, 7, 7, 0, 7, 0, 0]], np.int64)])
    one = np.array([0, 1], np.uint32)
    cases = [
        (dict(field=0, k=4), [1, 2, 3, 5], [20, 30, 40, 60], 4),
        (dict(field=0, descending=True, first=1, k=2), [3, 2], [40, 30], 4),
        (dict(field=0, k=4, req=(one, np.array([1], np.uint32))), [2, 3], [30, 40], 2),
        (dict(field=0, descending=True, k=4, mask_id=np.array([1], np.int32), ranges=(one, [(0, 25, 65)])), [5, 2], [60, 30], 2),
        (dict(field=1, descending=True, k=4), [1, 2, 3, 5], [7, 7, 7, 7], 4),
    ]
    for kw, docs, values, total in cases:
        d, v, n_out, n_match, _ = tm.field_topk(n_docs, title, body, q_ptr, q_terms, fields, masks=masks, **kw)
        assert (d[0].tolist(), v[0].tolist(), int(n_out[0]), int(n_match[0])) == (docs, values, len(docs), total), kw


# ---- the model against a per-doc sort -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [1, 2, 3])
def test_model_against_python_sort(seed):
    rng = np.random.default_rng(seed)
    n_docs, n_terms, n_q = 70, 12, 10
    title = csr(n_terms, {t: rng.choice(n_docs, rng.integers(0, 6), replace=False).tolist() for t in range(n_terms)})
    body = csr(n_terms, {t: rng.choice(n_docs, rng.integers(0, 30), replace=False).tolist() for t in range(n_terms)})
    masks = rng.random((3, n_docs)) < 0.6
    edge = np.array([I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX - 1, I64_MAX], np.int64)
    fields = np.stack([rng.integers(0, 8, n_docs), edge[rng.integers(0, len(edge), n_docs)]]).astype(np.int64)
    lens = rng.integers(0, 5, n_q)
    q_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    q_terms = rng.integers(0, n_terms + 2, int(q_ptr[-1])).astype(np.uint32)
    mask_id = rng.integers(-1, 3, n_q).astype(np.int32)
    ranges = (np.arange(n_q + 1, dtype=np.uint32), [(0, 1, 6) if q % 2 else (1, I64_MIN, I64_MAX) for q in range(n_q)])
    seen = 0
    for field in (0, 1):
        for desc in (False, True):
            for first, k in ((0, 1), (0, 5), (3, 4), (60, 5), (0, MAX_TOPK)):
                d, v, n_out, n_match, sets = tm.field_topk(n_docs, title, body, q_ptr, q_terms, fields, field, desc, first, k, masks=masks,
                                                           mask_id=mask_id, ranges=ranges)
                for q in range(n_q):
                    m = [x for x in range(n_docs) if sets[q][x]]

                    def before(x, y):           # the defined order, spelled out: value, then doc id ascending in both directions
                        vx, vy = int(fields[field][x]), int(fields[field][y])
                        if vx != vy:
                            return -1 if (vx > vy if desc else vx < vy) else 1
                        return -1 if x < y else 1

                    page = sorted(m, key=functools.cmp_to_key(before))[first:first + k]
                    assert d[q].tolist() == page and v[q].tolist() == [int(fields[field][x]) for x in page]
                    assert int(n_out[q]) == min(max(len(m) - first, 0), k) and int(n_match[q]) == len(m)
                    seen += len(page)
    assert seen > 500


# ---- field_topk_plan.hpp under the sanitizers -----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("field_topk_plan") / "field_topk_plan_harness")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "field_topk_plan_harness.cpp"), "-o", exe], check=True)
    return exe


def ask(harness, lines):
    r = subprocess.run([harness], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert out[-1] == f"ok {len(lines)} lines"
    return out[:-1]


EDGE = [I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX - 1, I64_MAX]


def test_plan_harness_key_transform(harness):
    """the key reads back to its value, keys of ascending values ascend, of descending values descend, and the order of (key, doc) pairs
    is the defined order of (value, doc) in both directions: docs of equal value by ascending doc id"""
    for desc in (0, 1):
        out = ask(harness, [f"k {v} {desc}" for v in EDGE])
        keys = [int(line.split()[0], 16) for line in out]
        assert [int(line.split()[1]) for line in out] == EDGE
        assert keys == sorted(keys, reverse=bool(desc)) and len(set(keys)) == len(keys)
    assert ask(harness, [f"k {I64_MIN} 0", f"k {I64_MAX} 0", f"k {I64_MAX} 1", f"k {I64_MIN} 1"]) == [
        f"{0:016x} {I64_MIN}", f"{2 ** 64 - 1:016x} {I64_MAX}", f"{0:016x} {I64_MAX}", f"{2 ** 64 - 1:016x} {I64_MIN}"]
    pairs = [(v, d) for v in EDGE for d in (0, 7, 2 ** 32 - 2)]
    for desc in (0, 1):
        lines, want = [], []
        for va, da in pairs:
            for vb, db in pairs:
                lines.append(f"c {va} {da} {vb} {db} {desc}")
                first = (va > vb if desc else va < vb) if va != vb else da < db
                want.append("1" if first else "0")
        assert ask(harness, lines) == want


def test_plan_harness_runs(harness):
    cus = 256
    cases = [(nb, na, forced) for nb in (1, 2, 3, 306) for na in (1, 7, 1024) for forced in (0, 1, 2, nb, nb + 5, 2 ** 40)]
    out = ask(harness, [f"r {nb} {na} {cus} {forced}" for nb, na, forced in cases])
    for (nb, na, forced), line in zip(cases, out):
        f = [int(x) for x in line.split()]
        R = f[0]
        assert f[1] == 1 and 1 <= R <= nb, (nb, na, forced, line)             # every run non-empty, the runs tile [0, n_blocks)
        if forced:
            assert R == min(forced, nb), (nb, na, forced, line)               # a forced R above n_blocks is clamped
        else:
            assert R == min(nb, 64, -(-64 * cus // na)), (nb, na, line)       # few queries: many runs; many queries: few
        assert f[2:] == [r * nb // R for r in range(min(R, 8))]
    assert ask(harness, ["r 0 5 256 0", "r 306 0 0 0"]) == ["0 1", "64 1 0 4 9 14 19 23 28 33"]


def test_plan_harness_buffer(harness):
    ks = [1, 2, 10, 100, 255, 256, 257, 512, 513, 1000, 1024]
    out = ask(harness, [f"b {K}" for K in ks])
    for K, line in zip(ks, out):
        entries, lds = (int(x) for x in line.split())
        assert entries & (entries - 1) == 0 and entries >= max(2 * K, 512) and entries < max(4 * K, 513) and lds == entries * 12, (K, line)
    assert out[0] == out[2] == "512 6144" and out[-1] == "2048 24576"          # the LDS follows K: a page of 10 takes a quarter of K = 1024


def test_plan_harness_groups_and_launches(harness):
    per = lambda R, K: R * (K * 12 + 8)                                         # noqa: E731
    cases = [(1024, 4, 1024, 0), (1024, 4, 1024, 3 * per(4, 1024)), (7, 2, 10, 1), (7, 2, 10, per(2, 10)), (7, 2, 10, 2 * per(2, 10) + 1),
             (1, 306, 1024, 100), (5, 3, 1, 10 ** 15), (0, 1, 1, 0)]
    out = ask(harness, [f"s {a} {R} {K} {opt}" for a, R, K, opt in cases])
    for (a, R, K, opt), line in zip(cases, out):
        group, n_groups, covered, bytes_q = (int(x) for x in line.split())
        scratch = opt if opt >= 1 else 256 << 20
        assert bytes_q == per(R, K) and covered == 1
        assert group == min(a, max(1, scratch // per(R, K))) and n_groups == (-(-a // group) if a else 0), (a, R, K, opt, line)
    assert [l.split()[:2] for l in out[:4]] == [["1024", "1"], ["3", "342"], ["1", "7"], ["1", "7"]]
    cuts = [(1, 1), (4, 1024), (306, 2 ** 31 - 1), (306, 2 ** 30), (64, 2 ** 26), (3, 2 ** 30 + 1), (0, 4), (4, 0)]
    out = ask(harness, [f"l {R} {n}" for R, n in cuts])
    for (R, n), line in zip(cuts, out):
        n_l, covered, max_grid = (int(x) for x in line.split())
        if R == 0 or n == 0:
            assert (n_l, covered) == (0, 1)
            continue
        per_l = max(1, (2 ** 31 - 1) // n)
        assert n_l == -(-R // per_l) and covered == 1 and max_grid <= 2 ** 31 - 1, (R, n, line)


def test_plan_harness_refusals(harness):
    #        n_q q_ptr docs_out n_out field first k n_fields
    cases = [((4, 1, 1, 1, 0, 0, 10, 1), OK), ((4, 1, 1, 1, 3, 1000, 24, 4), OK), ((4, 1, 1, 1, 0, 0, MAX_TOPK, 2), OK),
             ((4, 1, 1, 1, 1, MAX_TOPK - 1, 1, 2), OK), ((0, 0, 0, 0, 0, 0, 1, 1), OK),
             ((-1, 1, 1, 1, 0, 0, 10, 1), INVALID), ((4, 0, 1, 1, 0, 0, 10, 1), INVALID), ((4, 1, 0, 1, 0, 0, 10, 1), INVALID),
             ((4, 1, 1, 0, 0, 0, 10, 1), INVALID), ((4, 1, 1, 1, 0, 0, 0, 1), INVALID), ((4, 1, 1, 1, 0, 0, -5, 1), INVALID),
             ((4, 1, 1, 1, 0, -1, 10, 1), INVALID), ((4, 1, 1, 1, -1, 0, 10, 1), INVALID), ((4, 1, 1, 1, 1, 0, 10, 1), INVALID),
             ((4, 1, 1, 1, 4, 0, 10, 4), INVALID), ((4, 1, 1, 1, 2 ** 31 - 1, 0, 10, 4), INVALID),
             ((4, 1, 1, 1, 0, 0, MAX_TOPK + 1, 1), UNSUPPORTED), ((4, 1, 1, 1, 0, MAX_TOPK, 1, 1), UNSUPPORTED),
             ((4, 1, 1, 1, 0, 1000, 25, 1), UNSUPPORTED), ((4, 1, 1, 1, 0, 2 ** 31 - 1, 2 ** 31 - 1, 1), UNSUPPORTED),   # no overflow
             ((4, 1, 1, 1, 0, 0, 10, 0), STATE),
             # n_q == 0 is SS_OK whatever else is wrong: no field table, a page past SS_MAX_TOPK, k < 1, a bad field
             ((0, 0, 0, 0, 0, 0, 10, 0), OK), ((0, 0, 0, 0, 0, 1, MAX_TOPK, 1), OK), ((0, 0, 0, 0, 9, -1, 0, 1), OK)]
    out = ask(harness, [" ".join(["a"] + [str(x) for x in c]) for c, _ in cases])
    assert out == [str(code) for _, code in cases]
