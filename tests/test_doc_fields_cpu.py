"""CPU checks of the doc-field feature: hand-derived known answers for the model of the header's definitions (tests/doc_fields_model.py),
the header's new prototypes and constants under an unchanged SS_ABI_VERSION, sizeof(ss_doc_range) through a compiled C snippet, and
the kernel geometry the GPU test states."""
import os
import re
import subprocess

import numpy as np

from spaghettisearch_amd import engine
from tests import doc_fields_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spaghetti_rank.h")
I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1


def table70():
    """70 docs, two fields: field 0 cycles through INT64_MIN, -1, 0, INT64_MAX (doc d holds entry d % 4); field 1 = d"""
    cyc = np.array([I64_MIN, -1, 0, I64_MAX], np.int64)
    return np.stack([cyc[np.arange(70) % 4], np.arange(70, dtype=np.int64)])


def bits(docs, n_words):
    out = [0] * n_words
    for d in docs:
        out[d >> 5] |= 1 << (d & 31)
    return out


def test_set_words_known_answers():
    v = table70()
    every = list(range(70))
    sets = [[], [(0, -1, -1)], [(0, I64_MIN, I64_MIN)], [(0, I64_MAX, I64_MAX)], [(0, -1, 0)], [(0, I64_MIN, I64_MAX)], [(0, 1, -1)],
            [(1, 31, 33)], [(1, 64, 1000)], [(0, 0, I64_MAX), (1, 60, 69)], [(1, 0, 69), (1, 69, 0)]]
    want = [every, [d for d in every if d % 4 == 1], [d for d in every if d % 4 == 0], [d for d in every if d % 4 == 3],
            [d for d in every if d % 4 in (1, 2)], every, [], [31, 32, 33], [64, 65, 66, 67, 68, 69], [62, 63, 66, 67], []]
    got = fm.set_words(v, 70, sets)
    assert got.shape == (11, 3) and got.dtype == np.uint32
    assert got.tolist() == [bits(w, 3) for w in want]
    # the last word's dead bits: docs 64 .. 69 are bits 0 .. 5, bits 6 .. 31 stay 0 whatever matches
    assert got[0].tolist() == [0xFFFFFFFF, 0xFFFFFFFF, 0x3F] and got[5, 2] == 0x3F and got[8].tolist() == [0, 0, 0x3F]
    assert got[1, 0] == 0x22222222 and got[2, 0] == 0x11111111 and got[3, 0] == 0x88888888 and got[4, 0] == 0x66666666
    # a registered mask is the base: a set without clauses is its mask, -1 is every doc; the layout is pack_doc_masks'
    masks = np.zeros((2, 70), bool)
    masks[0, [0, 5, 31, 32, 69]] = True
    masks[1, :] = True
    got = fm.set_words(v, 70, [[], [(1, 5, 32)], [(1, 5, 32)], []], mask_id=[0, 0, -1, 1], masks=masks)
    assert got.tolist() == [bits([0, 5, 31, 32, 69], 3), bits([5, 31, 32], 3), bits(range(5, 33), 3), bits(every, 3)]
    assert fm.set_words(v, 70, [[], []], mask_id=[0, 1], masks=masks).tobytes() == engine.pack_doc_masks(masks, 70).tobytes()
    for n_docs in (1, 31, 32, 33, 64):
        assert fm.set_words(v[:, :n_docs], n_docs, [[]]).tolist() == [bits(range(n_docs), (n_docs + 31) // 32)]


def rows_of(docs):
    hits = np.zeros((1, len(docs)), engine.HIT_DTYPE)
    hits["doc"][0] = docs
    hits["final"][0] = np.arange(len(docs)) + 0.5          # marks the window position: nothing is sorted by it
    hits["_pad"][0] = 0xABCD
    return hits


def test_sort_page_known_answers():
    v = table70()                                            # field 0 of docs 0 .. 7: MIN, -1, 0, MAX, MIN, -1, 0, MAX
    docs = [3, 2, 70, 1, 0, 7, 0xFFFFFFFF, 6, 2, 4]          # positions 2 and 6 are outside the table; doc 2 twice
    hits, n_hits = rows_of(docs), np.array([10], np.int32)

    def page(desc, first, k, n=10):
        out = fm.sort_page(hits, np.array([n], np.int32), v, 70, 0, desc, first, k, np.zeros((1, k), engine.HIT_DTYPE), np.full(1, -7, np.int32),
                           np.full((1, k), 99, np.int64))
        cnt = int(out[1][0])
        assert (out[0]["_pad"][0, :cnt] == 0xABCD).all() and (out[0]["_pad"][0, cnt:] == 0).all() and (out[2][0, cnt:] == 99).all()
        return [int(x - 0.5) for x in out[0]["final"][0, :cnt]], out[2][0, :cnt].tolist()
    # ascending: MIN (positions 4, 9), -1 (3), 0 (1, 7, 8), MAX (0, 5), then the rows outside the table in window order
    assert page(False, 0, 10) == ([4, 9, 3, 1, 7, 8, 0, 5, 2, 6], [I64_MIN, I64_MIN, -1, 0, 0, 0, I64_MAX, I64_MAX, fm.NO_VALUE, fm.NO_VALUE])
    # descending: ties keep window order, the outside rows are still last
    assert page(True, 0, 10) == ([0, 5, 1, 7, 8, 3, 4, 9, 2, 6], [I64_MAX, I64_MAX, 0, 0, 0, -1, I64_MIN, I64_MIN, fm.NO_VALUE, fm.NO_VALUE])
    assert page(True, 3, 4)[0] == [7, 8, 3, 4] and page(False, 8, 5)[0] == [2, 6] and page(False, 9, 1)[0] == [6]
    assert page(False, 10, 3) == ([], []) and page(False, 11, 3) == ([], []) and page(True, 0, 3, n=0) == ([], [])
    assert page(False, 0, 10, n=3) == ([1, 0, 2], [0, I64_MAX, fm.NO_VALUE])
    # field 1 = the doc id: all distinct; the same doc twice stays in window order
    out = fm.sort_page(hits, n_hits, v, 70, 1, False, 0, 10, np.zeros((1, 10), engine.HIT_DTYPE), np.zeros(1, np.int32))
    assert out[0]["doc"][0].tolist() == [0, 1, 2, 2, 3, 4, 6, 7, 70, 0xFFFFFFFF] and out[0]["final"][0, 2] == 1.5 and out[2] is None
    # clamped counts (what the kernel does with a device n_hits)
    bad = fm.sort_page(hits, np.array([99], np.int32), v, 70, 1, False, 0, 10, np.zeros((1, 10), engine.HIT_DTYPE), np.zeros(1, np.int32), clamp=True)
    assert bad[1][0] == 10 and bad[0].tobytes() == out[0].tobytes()
    assert fm.sort_page(hits, np.array([-5], np.int32), v, 70, 1, False, 0, 10, np.zeros((1, 10), engine.HIT_DTYPE), np.ones(1, np.int32), clamp=True)[1][0] == 0


def test_gather_known_answers():
    v = table70()
    hits = rows_of([3, 70, 0, 69, 5])
    out = fm.gather(hits, np.array([4], np.int32), v, 70, np.full((1, 5, 2), 99, np.int64))
    assert out[0].tolist() == [[I64_MAX, 3], [fm.NO_VALUE, fm.NO_VALUE], [I64_MIN, 0], [-1, 69], [99, 99]]
    assert fm.NO_VALUE == I64_MIN                            # an ordinary value otherwise: doc 0 holds it in field 0


def test_header_carries_the_new_entry_points_under_abi_4():
    text = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"#define SS_ABI_VERSION 4\b", code)
    for name, n_params in (("ss_scorer_set_doc_fields", 3), ("ss_doc_field_masks", 6), ("ss_score_topk_filtered", 18),
                           ("ss_sort_hits_by_field", 12), ("ss_hit_fields", 6)):
        m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*?)\)\s*;", code, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == n_params, name
    assert re.search(r"#define SS_MAX_DOC_FIELDS 4\b", code) and re.search(r"#define SS_MAX_RANGE_CLAUSES 4\b", code)
    assert re.search(r"#define SS_NO_FIELD_VALUE INT64_MIN\b", code)
    assert fm.MAX_FIELDS == 4 and fm.MAX_CLAUSES == 4
    from spaghettisearch_amd import _lib
    assert (_lib.SS_MAX_DOC_FIELDS, _lib.SS_MAX_RANGE_CLAUSES, _lib.SS_NO_FIELD_VALUE) == (4, 4, I64_MIN)
    for name in ("ss_scorer_set_doc_fields", "ss_doc_field_masks", "ss_score_topk_filtered", "ss_sort_hits_by_field", "ss_hit_fields"):
        assert name in _lib.PROTOTYPES


def test_doc_range_is_24_bytes(tmp_path):
    import ctypes
    from spaghettisearch_amd import _lib
    src = tmp_path / "range_size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "spaghetti_rank.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(ss_doc_range), offsetof(ss_doc_range, field), '
                   'offsetof(ss_doc_range, lo), offsetof(ss_doc_range, hi)); return SS_NO_FIELD_VALUE < 0 ? 0 : 1; }\n')
    exe = tmp_path / "range_size"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert out == ["24", "0", "8", "16"]
    assert ctypes.sizeof(_lib.SsDocRange) == 24 == engine.DOC_RANGE_DTYPE.itemsize
    assert [engine.DOC_RANGE_DTYPE.fields[n][1] for n in ("field", "_pad", "lo", "hi")] == [0, 4, 8, 16]
    ptr, rng = engine.pack_doc_ranges([[(1, -5, 7)], [], [(0, I64_MIN, I64_MAX), (3, 2, 1)]])
    assert ptr.tolist() == [0, 1, 1, 3] and rng["field"].tolist() == [1, 0, 3] and rng["lo"].tolist() == [-5, I64_MIN, 2]
    assert rng["hi"].tolist() == [7, I64_MAX, 1] and (rng["_pad"] == 0).all()


def test_kernel_geometry_the_gpu_test_states():
    """tests/test_gpu_doc_fields.py states B = FM_DOCS and G = FM_GROUP of csrc/field.hip: derived here from the file's constants"""
    src = open(os.path.join(ROOT, "spaghettisearch_amd", "csrc", "field.hip")).read()
    const = {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr int (FM_[A-Z_]+) = (\d+);", src)}
    docs = (const["FM_TPB"] // 64) * const["FM_STEPS"] * 64
    assert "FM_DOCS = (FM_TPB / 64) * FM_WAVE_DOCS" in src and "FM_WAVE_DOCS = FM_STEPS * 64" in src
    gpu_test = open(os.path.join(ROOT, "tests", "test_gpu_doc_fields.py")).read()
    assert re.search(r"^B = (\d+)", gpu_test, flags=re.M).group(1) == str(docs) and docs <= 32768
    assert re.search(r"^G = (\d+)", gpu_test, flags=re.M).group(1) == str(const["FM_GROUP"])
