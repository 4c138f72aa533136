"""CPU checks of near-duplicate results: the numpy model (tests/dedup_model.py) on the header's known answers and on hand-written
cases, and the four new entry points in the header and in the binding.  No GPU."""
import itertools
import os
import re

import numpy as np
import pytest

from tests import dedup_model as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spaghetti_rank.h")
NEW = {"ss_index_build_signatures": 2, "ss_index_drop_signatures": 1, "ss_index_read_signatures": 5, "ss_dedup_hits": 12}

KNOWN = [(0, 0, 0x92CA2F0E), (1, 0, 0x96A0F96B), (0, 1, 0x3CD6E3F3), (12345, 3, 0x8EE55794), (0xFFFFFFFE, 31, 0x26D56D90),
         (70000, 15, 0x231FE950)]


def test_hash_known_answers_in_both_implementations():
    for t, s, want in KNOWN:
        assert dm.h_int(t, s) == want, (t, s, hex(dm.h_int(t, s)))
        assert int(dm.h(t, s)) == want, (t, s)
    rng = np.random.default_rng(5)
    t = rng.integers(0, 2**32, 4000, dtype=np.uint64).astype(np.uint32)
    s = rng.integers(0, dm.MAX_SIG_SLOTS, 4000).astype(np.uint32)
    assert dm.h(t, s).tolist() == [dm.h_int(int(a), int(b)) for a, b in zip(t, s)]


def test_header_states_the_known_answers():
    text = open(HEADER).read()
    for _, _, want in KNOWN:
        assert f"0x{want:08X}" in text
    for want in (0x2316A329, 0x2C85567E, 0x41B9D641, 0x343B1A79):
        assert f"0x{want:08X}" in text


def test_signature_of_the_headers_row():
    assert dm.row_signature([3, 7, 70000], 4).tolist() == [0x2316A329, 0x2C85567E, 0x41B9D641, 0x343B1A79]
    assert [min(dm.h_int(t, s) for t in (3, 7, 70000)) for s in range(4)] == [0x2316A329, 0x2C85567E, 0x41B9D641, 0x343B1A79]
    assert dm.row_signature([], 8).tolist() == [dm.SIG_EMPTY] * 8


def test_signature_ignores_order_and_repeats():
    rng = np.random.default_rng(7)
    for n_slots in (4, 16, 32):
        row = rng.integers(0, 70000, 37).astype(np.uint32)
        want = dm.row_signature(row, n_slots)
        for _ in range(5):
            assert np.array_equal(dm.row_signature(rng.permutation(row), n_slots), want)
        assert np.array_equal(dm.row_signature(np.concatenate([row, row[:9], row[-1:]]), n_slots), want)
        assert np.array_equal(dm.row_signature(sorted(set(row.tolist())), n_slots), want)


def test_signatures_from_a_view_equal_the_rows_one_by_one():
    rng = np.random.default_rng(9)
    lens = [0, 3, 0, 1, 40, 0]
    rows = [np.sort(rng.choice(5000, n, replace=False)).astype(np.uint32) for n in lens]
    doc_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    doc_term = np.concatenate(rows).astype(np.uint32)
    for n_slots in (4, 32):
        sig = dm.signatures(doc_ptr, doc_term, n_slots)
        for d, row in enumerate(rows):
            assert np.array_equal(sig[d], dm.row_signature(row, n_slots)), d
    assert dm.signatures(np.zeros(4, np.uint64), np.zeros(0, np.uint32), 8).tolist() == [[dm.SIG_EMPTY] * 8] * 3


@pytest.mark.parametrize("n_slots", [4, 32])
def test_single_term_rows_never_have_the_empty_signature(n_slots):
    """empty signature <=> empty row: a one-term row is the row that comes closest to all SIG_EMPTY"""
    ids = np.concatenate([np.arange(6000), np.arange(2**32 - 3000, 2**32), [0x61C88646 - 1, 0x61C88646, 0x61C88647]]).astype(np.uint32)
    hv = dm.h(ids[:, None], np.arange(n_slots, dtype=np.uint32)[None, :])
    assert not np.any(np.all(hv == dm.SIG_EMPTY, axis=1))
    assert np.all((hv == dm.SIG_EMPTY).sum(axis=1) <= 1)          # no term reaches 0xFFFFFFFF in two slots
    # the mix is a bijection: the one pre-image of 0xFFFFFFFF, found by undoing it, is reached by exactly one term per slot
    inv1, inv2, m = pow(0x85EBCA6B, -1, 2**32), pow(0xC2B2AE35, -1, 2**32), 0xFFFFFFFF
    x = 0xFFFFFFFF
    x ^= x >> 16
    x = (x * inv2) & m
    x ^= (x >> 13) ^ (x >> 26)
    x = (x * inv1) & m
    x ^= x >> 16
    for s in range(n_slots):
        t = (x - 0x9E3779B9 * (s + 1)) & m
        assert dm.h_int(t, s) == dm.SIG_EMPTY
        assert [dm.h_int(t, s2) == dm.SIG_EMPTY for s2 in range(n_slots)].count(True) == 1


def M(n, pairs, own=()):
    """a symmetric match matrix: 10 on the diagonal, `pairs` {(i, j): match}, 0 elsewhere, -1 in the rows and columns of `own`"""
    m = np.zeros((n, n), dtype=np.int64)
    np.fill_diagonal(m, 10)
    for (i, j), v in pairs.items():
        m[i, j] = m[j, i] = v
    for o in own:
        m[o, :] = -1
        m[:, o] = -1
    return m


def test_walk_chain_drops_the_middle_only():
    kept, leader, similar = dm.walk(M(3, {(0, 1): 5, (1, 2): 5, (0, 2): 4}), 5)
    assert kept == [0, 2] and leader == [0, 0, 2] and similar == [2, 0, 1]
    kept, leader, similar = dm.walk(M(3, {(0, 1): 5, (1, 2): 5, (0, 2): 4}), 4)          # at 4 everything follows row 0
    assert kept == [0] and leader == [0, 0, 0] and similar == [3, 0, 0]


def test_walk_smallest_kept_leader_wins_and_a_dropped_row_leads_nothing():
    # rows 0 and 2 both match 3; 1 matches 3 as well but is dropped (it follows 0)
    kept, leader, _ = dm.walk(M(4, {(0, 1): 9, (1, 3): 9, (2, 3): 9, (0, 3): 9}), 9)
    assert kept == [0, 2] and leader == [0, 0, 2, 0]
    kept, leader, _ = dm.walk(M(4, {(0, 1): 9, (1, 3): 9, (2, 3): 9}), 9)
    assert kept == [0, 2] and leader == [0, 0, 2, 2]                                     # not 1: it was dropped


def test_walk_leader_in_an_earlier_tile_of_64():
    n = 130
    kept, leader, similar = dm.walk(M(n, {(3, 70): 7, (70, 129): 7, (64, 129): 7, (3, 64): 6}), 7)
    assert leader[70] == 3 and leader[129] == 64 and len(kept) == n - 2
    assert similar[3] == 2 and similar[64] == 2 and similar[70] == 0


def test_walk_rows_on_their_own_never_match_even_with_equal_docs():
    sig = np.array([[1, 2, 3, 4], [dm.SIG_EMPTY] * 4, [1, 2, 3, 9]], dtype=np.uint32)
    docs = [1, 1, 7, 7, 0, 0, 2]                                                         # doc 1: empty signature; doc 7: outside the table
    m = dm.match_matrix(docs, sig)
    assert np.array_equal(m, dm.fast_match(docs, sig))
    assert m[0, 1] == -1 and m[0, 0] == -1 and m[2, 3] == -1 and m[4, 5] == 4 and m[4, 6] == 3
    kept, leader, similar = dm.walk(m, 1)
    assert kept == [0, 1, 2, 3, 4] and leader == [0, 1, 2, 3, 4, 4, 4] and similar == [1, 1, 1, 1, 3, 0, 0]
    kept, _, _ = dm.walk(m, 4)
    assert kept == [0, 1, 2, 3, 4, 6]


def test_dedup_pages_and_untouched_tails():
    sig = np.arange(40, dtype=np.uint32).reshape(10, 4)
    sig[5] = sig[2]
    sig[8] = sig[2]
    hits = np.zeros((1, 10), dtype=dm.HIT_DTYPE)
    hits["doc"][0] = np.arange(10)
    hits["final"][0] = np.arange(10, 0, -1)
    for first, want in ((0, [0, 1, 2]), (3, [3, 4, 6]), (6, [7, 9]), (8, []), (11, [])):
        out = np.zeros((1, 3), dtype=dm.HIT_DTYPE)
        out["doc"] = 777
        n_out, sim, kept = np.full(1, -1, np.int32), np.full((1, 3), 99, np.uint32), np.full(1, -1, np.int32)
        dm.dedup(hits, np.array([10], np.int32), sig, 4, first, 3, out, n_out, sim, kept)
        assert n_out[0] == len(want) and kept[0] == 8
        assert out["doc"][0, :len(want)].tolist() == want and out["doc"][0, len(want):].tolist() == [777] * (3 - len(want))
        assert sim[0, :len(want)].tolist() == [3 if d == 2 else 1 for d in want] and sim[0, len(want):].tolist() == [99] * (3 - len(want))
    with pytest.raises(ValueError):
        dm.dedup(hits, np.array([11], np.int32), sig, 4, 0, 3, out, n_out)
    dm.dedup(hits, np.array([11], np.int32), sig, 4, 0, 3, out, n_out, clamp=True)
    assert n_out[0] == 3


def test_walk_agrees_with_the_definition_by_brute_force():
    """every symmetric 0/1 relation on 5 rows: j is dropped iff a KEPT i < j is related to it, and the leader is the smallest such i"""
    pairs = list(itertools.combinations(range(5), 2))
    for bits in range(1 << len(pairs)):
        m = M(5, {p: 1 for b, p in enumerate(pairs) if bits >> b & 1})
        kept, leader, _ = dm.walk(m, 1)
        is_kept = [True] * 5
        for j in range(5):
            cands = [i for i in range(j) if is_kept[i] and m[i, j] >= 1]
            is_kept[j] = not cands
            assert leader[j] == (min(cands) if cands else j)
        assert kept == [j for j in range(5) if is_kept[j]]


def _header_prototypes():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\bint32_t\s+(ss_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        params = m.group(2).strip()
        out[m.group(1)] = 0 if params in ("", "void") else params.count(",") + 1
    return out


def test_header_and_binding_declare_the_new_entry_points():
    from spaghettisearch_amd import _lib, engine
    protos = _header_prototypes()
    for name, n_args in NEW.items():
        assert protos.get(name) == n_args, name
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == n_args, name
    text = open(HEADER).read()
    assert re.search(r"#define SS_MAX_SIG_SLOTS 32\b", text) and re.search(r"#define SS_SIG_EMPTY 0xFFFFFFFFu", text)
    assert _lib.SS_MAX_SIG_SLOTS == dm.MAX_SIG_SLOTS == 32 and _lib.SS_SIG_EMPTY == dm.SIG_EMPTY
    assert re.search(r"#define SS_ABI_VERSION 4\b", text)
    for meth in ("build_signatures", "drop_signatures", "read_signatures"):
        assert callable(getattr(engine.InvertedIndex, meth))
    assert callable(engine.Scorer.dedup_hits)
