"""CPU checks of ss_top_groups' definition (tests/group_topk_model.py): the header's hand-worked known answer in its five forms, the model
against a plain per-doc Python count on random small tables, group_topk_plan.hpp driven on the host under ASan + UBSan
(tests/group_topk_plan_harness.cpp): the key at the ends of the count and rank ranges, the choice of the counting path, the stride of a
counter row, the groups of queries under a scratch bound, the runs and launches reused from field_topk_plan.hpp and every refusal of
the call's own arguments with its code; then the header itself: prototypes, the size of ss_group_count from a compiled C snippet, the
ABI version, and the refusals that need no device."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from spaghettisearch_amd import _lib
from tests import group_topk_model as gm
from tests.test_facet_cpu import csr, header_world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spaghettisearch_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "spaghetti_rank.h")
UNKNOWN = 0xFFFFFFFF
NO_GROUP = 0xFFFFFFFF
OK, INVALID, UNSUPPORTED, STATE = 0, 1, 2, 3
MAX_TOPK = 1024
HEADER_GROUPS = np.array([7, 7, 7, 3, 3, NO_GROUP, 0xFFFFFFFE, 3], np.uint32)


# ---- the known answer of the header ---------------------------------------------------------------------------------------------------

def test_header_known_answer():
    n_docs, title, body, fields, masks, _, q_ptr, q_terms = header_world()
    assert gm.group_values(HEADER_GROUPS).tolist() == [3, 7, 0xFFFFFFFE]
    one = np.array([0, 1], np.uint32)
    t2 = (np.array([0, 1], np.uint32), np.array([2], np.uint32))
    cases = [
        #  arguments                                 M             rows              n_groups n_ungrouped n_match
        (dict(first=0, m=4), [1, 2, 3, 5], [(7, 2), (3, 1)], 2, 1, 4),
        (dict(first=1, m=1), [1, 2, 3, 5], [(3, 1)], 2, 1, 4),
        (dict(first=0, m=4, req=(one, np.array([1], np.uint32))), [2, 3], [(3, 1), (7, 1)], 2, 0, 2),
        (dict(first=0, m=4, mask_id=np.array([1], np.int32), ranges=(one, [(0, 25, 65)])), [2, 5], [(7, 1)], 1, 1, 2),
        (dict(first=0, m=4, q=t2), [6], [(0xFFFFFFFE, 1)], 1, 0, 1),
    ]
    for kw, docs, rows, n_groups, n_ungrouped, n_match in cases:
        qp, qt = kw.pop("q", (q_ptr, q_terms))
        got = gm.top_groups(n_docs, title, body, qp, qt, HEADER_GROUPS, masks=masks, fields=fields, **kw)
        assert np.nonzero(got[5][0])[0].tolist() == docs, kw
        assert [tuple(r) for r in got[0][0].tolist()] == rows, kw
        assert (int(got[1][0]), int(got[2][0]), int(got[3][0]), int(got[4][0])) == (len(rows), n_groups, n_ungrouped, n_match), kw


# ---- the model against a per-doc count ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [1, 2, 3])
def test_model_against_doc_loop(seed):
    rng = np.random.default_rng(seed)
    n_docs, n_terms, n_q = 90, 12, 10
    title = csr(n_terms, {t: rng.choice(n_docs, rng.integers(0, 6), replace=False).tolist() for t in range(n_terms)})
    body = csr(n_terms, {t: rng.choice(n_docs, rng.integers(0, 40), replace=False).tolist() for t in range(n_terms)})
    masks = rng.random((3, n_docs)) < 0.7
    fields = rng.integers(0, 8, (1, n_docs)).astype(np.int64)
    values = np.array([0, 1, 5, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, NO_GROUP], np.uint32)
    group = values[rng.integers(0, len(values), n_docs)]
    lens = rng.integers(0, 5, n_q)
    q_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    q_terms = rng.integers(0, n_terms + 2, int(q_ptr[-1])).astype(np.uint32)
    mask_id = rng.integers(-1, 3, n_q).astype(np.int32)
    ranges = (np.arange(n_q + 1, dtype=np.uint32), [(0, 1, 6) if q % 2 else (0, 0, 7) for q in range(n_q)])
    seen = ties = 0
    for first, m in ((0, 1), (0, 3), (2, 2), (6, 5), (0, MAX_TOPK)):
        rows, n_out, n_groups, n_ungrouped, n_match, sets = gm.top_groups(n_docs, title, body, q_ptr, q_terms, group, first, m, masks=masks,
                                                                          fields=fields, mask_id=mask_id, ranges=ranges)
        for q in range(n_q):
            cnt, ungrouped, total = {}, 0, 0
            for d in range(n_docs):
                if not sets[q][d]:
                    continue
                total += 1
                if int(group[d]) == NO_GROUP:
                    ungrouped += 1
                else:
                    cnt[int(group[d])] = cnt.get(int(group[d]), 0) + 1
            every = sorted(cnt.items(), key=lambda vc: (-vc[1], vc[0]))       # count descending, value ascending as unsigned
            assert [tuple(r) for r in rows[q].tolist()] == every[first:first + m]
            assert (int(n_out[q]), int(n_groups[q]), int(n_ungrouped[q]), int(n_match[q])) == \
                (min(max(len(every) - first, 0), m), len(every), ungrouped, total)
            assert sum(cnt.values()) + ungrouped == total
            seen += len(rows[q])
            ties += len(every) - len({c for _, c in every})
    assert seen > 60 and ties > 10


# ---- group_topk_plan.hpp under the sanitizers -----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("group_topk_plan") / "group_topk_plan_harness")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "group_topk_plan_harness.cpp"), "-o", exe], check=True)
    return exe


def ask(harness, lines):
    r = subprocess.run([harness], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert out[-1] == f"ok {len(lines)} lines"
    return out[:-1]


def test_plan_harness_key(harness):
    """the key reads back to count and rank at the ends of both ranges, and ascending keys are the defined order: count descending, equal
    counts by rank ascending"""
    n_groups = 2 ** 32 - 1                                                      # the most distinct values != SS_NO_GROUP there can be
    pairs = [(c, r) for c in (1, 2, 1000, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1) for r in (0, 1, 4095, n_groups - 1)]
    out = ask(harness, [f"k {c} {r}" for c, r in pairs])
    keys = []
    for (c, r), line in zip(pairs, out):
        key, c_back, r_back = line.split()
        assert (int(c_back), int(r_back)) == (c, r) and int(key, 16) == ((0xFFFFFFFF - c) << 32 | r)
        keys.append(int(key, 16))
    assert max(keys) < 2 ** 64 - 1                                              # the pad key is no group's key
    by_key = [p for _, p in sorted(zip(keys, pairs))]
    assert by_key == sorted(pairs, key=lambda cr: (-cr[0], cr[1])) and len(set(keys)) == len(keys)
    assert out[0] == f"{0xFFFFFFFE00000000:016x} 1 0" and out[-1] == f"{n_groups - 1:016x} {2 ** 32 - 1} {n_groups - 1}"


def test_plan_harness_path_and_row(harness):
    cases = [(0, 8192), (1, 8192), (64, 8192), (8192, 8192), (8193, 8192), (100000, 8192), (64, 0), (64, -1), (64, 63), (64, 64), (5, 1),
             (8192, 2 ** 40), (8193, 2 ** 40), (2 ** 32 - 1, 2 ** 40)]
    out = ask(harness, [f"p {n} {o}" for n, o in cases])
    for (n, o), line in zip(cases, out):
        use, lds = (int(x) for x in line.split())
        assert use == int(o > 0 and n <= o and n <= 8192), (n, o, line)          # 0 means never; the histogram holds at most 8192 counters
        if use:
            assert lds % 16 == 0 and n * 4 <= lds < n * 4 + 16 and lds <= 32768
    sizes = [0, 1, 2, 3, 5, 6, 7, 64, 8192, 65573, 100000, 2 ** 32 - 2, 2 ** 32 - 1]
    out = ask(harness, [f"w {n}" for n in sizes])
    for n, line in zip(sizes, out):
        stride, s_match, s_ungrouped = (int(x) for x in line.split())
        assert stride % 4 == 0 and n + 2 <= stride < n + 6, (n, line)             # the two extra slots inside, rows 16-byte aligned
        assert (s_match, s_ungrouped) == (n, n + 1)
    assert out[:4] == ["4 0 1", "4 1 2", "4 2 3", "8 3 4"]
    ks = [1, 10, 256, 257, 1024]
    out = ask(harness, [f"b {K}" for K in ks])
    for K, line in zip(ks, out):
        entries, lds = (int(x) for x in line.split())
        assert entries & (entries - 1) == 0 and entries >= max(2 * K, 512) and lds == entries * 8, (K, line)


def test_plan_harness_groups_runs_and_launches(harness):
    row = lambda n: (n + 2 + 3) // 4 * 16                                       # noqa: E731  (bytes of a counter row)
    cases = [(1024, 64, 0), (1024, 100000, 0), (1024, 100000, 3 * row(100000)), (7, 5, 1), (7, 5, row(5)), (7, 5, 2 * row(5) + 1),
             (14, 65573, 1000), (1, 2 ** 32 - 1, 100), (5, 3, 10 ** 15), (0, 1, 0), (3000, 2 ** 32 - 1, 0)]
    out = ask(harness, [f"s {a} {n} {opt}" for a, n, opt in cases])
    for (a, n, opt), line in zip(cases, out):
        group, n_launch_groups, covered, row_bytes = (int(x) for x in line.split())
        scratch = opt if opt >= 1 else 256 << 20
        assert row_bytes == row(n) and covered == 1
        assert group == min(a, max(1, scratch // row(n))) and n_launch_groups == (-(-a // group) if a else 0), (a, n, opt, line)
    #       a row larger than the bound goes alone: one query per group
    assert [l.split()[:2] for l in out[:4]] == [["1024", "1"], ["671", "2"], ["3", "342"], ["1", "7"]]
    assert out[6].split()[:2] == ["1", "14"] and out[10].split()[:2] == ["1", "3000"]
    runs = [(nb, na, forced) for nb in (1, 3, 306) for na in (1, 14, 1024) for forced in (0, 1, 3, nb + 5)]
    out = ask(harness, [f"r {nb} {na} 256 {forced}" for nb, na, forced in runs])
    for (nb, na, forced), line in zip(runs, out):
        f = [int(x) for x in line.split()]
        assert f[1] == 1 and f[0] == (min(forced, nb) if forced else min(nb, 64, -(-64 * 256 // na))), (nb, na, forced, line)
        assert f[2:] == [r * nb // f[0] for r in range(min(f[0], 8))]
    cuts = [(1, 1), (3, 14), (306, 2 ** 31 - 1), (64, 2 ** 26), (0, 4), (4, 0)]
    out = ask(harness, [f"l {R} {n}" for R, n in cuts])
    for (R, n), line in zip(cuts, out):
        n_l, covered, max_grid = (int(x) for x in line.split())
        if R == 0 or n == 0:
            assert (n_l, covered) == (0, 1)
            continue
        assert n_l == -(-R // max(1, (2 ** 31 - 1) // n)) and covered == 1 and max_grid <= 2 ** 31 - 1, (R, n, line)


def test_plan_harness_refusals(harness):
    #        n_q q_ptr groups_out n_out first m has_table
    cases = [((4, 1, 1, 1, 0, 10, 1), OK), ((4, 1, 1, 1, 1000, 24, 1), OK), ((4, 1, 1, 1, 0, MAX_TOPK, 1), OK), ((4, 1, 1, 1, MAX_TOPK - 1, 1, 1), OK),
             ((-1, 1, 1, 1, 0, 10, 1), INVALID), ((4, 0, 1, 1, 0, 10, 1), INVALID), ((4, 1, 0, 1, 0, 10, 1), INVALID),
             ((4, 1, 1, 0, 0, 10, 1), INVALID), ((4, 1, 1, 1, 0, 0, 1), INVALID), ((4, 1, 1, 1, 0, -5, 1), INVALID),
             ((4, 1, 1, 1, -1, 10, 1), INVALID),
             ((4, 1, 1, 1, 0, MAX_TOPK + 1, 1), UNSUPPORTED), ((4, 1, 1, 1, MAX_TOPK, 1, 1), UNSUPPORTED), ((4, 1, 1, 1, 1000, 25, 1), UNSUPPORTED),
             ((4, 1, 1, 1, 2 ** 31 - 1, 2 ** 31 - 1, 1), UNSUPPORTED),                                                    # no overflow
             ((4, 1, 1, 1, 0, 10, 0), STATE),
             # n_q == 0 is SS_OK whatever else is wrong: no table, a page past SS_MAX_TOPK, m < 1, NULL arrays
             ((0, 0, 0, 0, 0, 10, 0), OK), ((0, 0, 0, 0, 1, MAX_TOPK, 1), OK), ((0, 0, 0, 0, -1, 0, 1), OK)]
    out = ask(harness, [" ".join(["a"] + [str(x) for x in c]) for c, _ in cases])
    assert out == [str(code) for _, code in cases]


# ---- the header and the library, without a device -------------------------------------------------------------------------------------

def test_header_prototypes_struct_size_and_abi_version(tmp_path):
    text = open(HEADER).read()
    assert re.search(r"^#define SS_ABI_VERSION 4$", text, re.M)
    block = text[:text.index("#define SS_ABI_VERSION")]
    for name in ("ss_group_count", "ss_scorer_group_values", "ss_top_groups"):
        assert name in block, name                                               # the ABI comment block names what was added under 4
    assert re.search(r"int32_t ss_scorer_group_values\(ss_scorer\* s, uint32_t\* n_groups_out[^;]*uint32_t\* values_out [^)]*\);", text)
    proto = re.search(r"int32_t ss_top_groups\(([^;]*)\);", text).group(1)
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", proto).split(",")]
    assert [p.split()[-1] for p in params] == ["s", "n_q", "q_ptr", "q_terms", "mask_id", "req_ptr", "req_terms", "exc_ptr", "exc_terms", "rng_ptr",
                                               "rng", "first", "m", "groups_out", "n_out", "n_groups_out", "n_ungrouped_out", "n_match_out"]
    assert params[13].startswith("ss_group_count*") and params[11] == "int32_t first" and params[12] == "int32_t m"
    assert len(_lib.PROTOTYPES["ss_top_groups"][1]) == len(params) and len(_lib.PROTOTYPES["ss_scorer_group_values"][1]) == 3
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "spaghetti_rank.h"\n'
                   'int main(void) { printf("%zu %zu %zu %d\\n", sizeof(ss_group_count), offsetof(ss_group_count, group), '
                   'offsetof(ss_group_count, count), SS_ABI_VERSION); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["8", "0", "4", "4"]
    assert gm.GROUP_COUNT_DTYPE.itemsize == 8
    from spaghettisearch_amd import engine
    assert engine.GROUP_COUNT_DTYPE == gm.GROUP_COUNT_DTYPE


def test_refusals_without_a_device():
    """a NULL handle is refused before anything looks for a device"""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libspaghetti_rank.so is not built")
    lib = _lib.load()
    assert lib.ss_abi_version() == 4
    buf = (ctypes.c_uint32 * 8)()
    p = ctypes.addressof(buf)
    assert lib.ss_top_groups(None, 1, p, p, None, None, None, None, None, None, None, 0, 1, p, p, None, None, None) == INVALID
    assert lib.ss_top_groups(None, 0, None, None, None, None, None, None, None, None, None, 0, 1, None, None, None, None, None) == INVALID
    assert lib.ss_scorer_group_values(None, p, None) == INVALID
    assert bytes(buf) == bytes(32)
