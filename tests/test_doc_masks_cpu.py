"""CPU checks of the doc allow-list boundary (ss_scorer_set_doc_masks, ss_score_topk_masked): the header declares both entry
points, the library exports them, a C99 caller that uses them compiles and links, and engine.pack_doc_masks packs like numpy."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spaghetti_rank.h")
SYMS = ("ss_scorer_set_doc_masks", "ss_score_topk_masked")


def _lib_path():
    from spaghettisearch_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.LIB_PATH


def test_header_declares_and_library_exports_the_mask_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for s in SYMS:
        assert re.search(r"\bint32_t\s+" + s + r"\s*\(", text), s
    lib = ctypes.CDLL(_lib_path())
    for s in SYMS:
        assert hasattr(lib, s), s
    from spaghettisearch_amd import _lib
    assert all(s in _lib.PROTOTYPES for s in SYMS)


C_CALLER = r"""
#include <stdio.h>
#include <stdlib.h>
#include "spaghetti_rank.h"

int main(void) {
    ss_ctx* ctx = NULL;
    if (ss_init(0, &ctx) != SS_OK) { printf("no device\n"); return 0; }
    ss_scorer* sc = NULL;
    uint32_t words[2] = {0x5u, 0x1u};
    const uint32_t q_ptr[2] = {0, 1}, q_terms[1] = {0};
    const int32_t mask_id[1] = {1};
    ss_hit hits[4];
    int32_t n_hits[1];
    int32_t rc = ss_scorer_set_doc_masks(sc, 2, words);
    rc |= ss_score_topk_masked(sc, 1, q_ptr, q_terms, NULL, NULL, NULL, NULL, mask_id, 4, hits, n_hits);
    ss_shutdown(ctx);
    return rc == SS_OK;     /* a NULL scorer must be refused */
}
"""


def test_c99_caller_compiles_and_links(tmp_path):
    lib = _lib_path()
    src = tmp_path / "masks.c"
    src.write_text(C_CALLER)
    exe = tmp_path / "masks"
    subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", os.path.dirname(lib), "-lspaghetti_rank", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert exe.exists()


@pytest.mark.parametrize("n_docs", [1, 31, 32, 33, 64, 1000, 4097])
def test_pack_doc_masks_matches_numpy(n_docs):
    from spaghettisearch_amd import engine
    rng = np.random.default_rng(n_docs)
    dense = rng.random((4, n_docs)) < np.array([[0.0], [0.5], [0.1], [1.0]])
    words = engine.pack_doc_masks(dense, n_docs)
    n_words = (n_docs + 31) // 32
    assert words.dtype == np.uint32 and words.shape == (4, n_words)
    padded = np.zeros((4, n_words * 32), dtype=bool)
    padded[:, :n_docs] = dense
    ref = np.packbits(padded, axis=1, bitorder="little").view("<u4")
    assert np.array_equal(words, ref)
    for m in range(4):                                          # bit (d & 31) of word d >> 5 = doc d
        d = np.arange(n_docs)
        assert np.array_equal((words[m][d >> 5] >> (d & 31)) & 1, dense[m].astype(np.uint32))
    if n_docs % 32:                                             # bits past n_docs stay clear
        assert not (words[:, -1] >> np.uint32(n_docs % 32)).any()
    # the same sets as doc-id lists
    sets = [np.nonzero(dense[m])[0] for m in range(4)]
    assert np.array_equal(engine.pack_doc_masks(sets, n_docs), words)


def test_pack_doc_masks_rejects_bad_input():
    from spaghettisearch_amd import engine
    with pytest.raises(ValueError):
        engine.pack_doc_masks([np.array([5])], 5)
    with pytest.raises(ValueError):
        engine.pack_doc_masks([np.array([-1])], 5)
    with pytest.raises(ValueError):
        engine.pack_doc_masks(np.zeros((2, 4), dtype=bool), 5)
    assert engine.pack_doc_masks([], 10).shape == (0, 1)
