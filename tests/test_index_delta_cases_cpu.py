"""CPU evidence for tests/index_delta_cases.py: every case stands on the path it names, the model (tests/index_delta_model.py)
behaves as the header says, and a second, independent statement of the merge - sort the surviving and the new (term, doc) keys
with numpy - gives the same arrays.  No GPU, no library."""
from fractions import Fraction

import numpy as np
import pytest

from tests import index_delta_cases as dc
from tests.index_delta_model import REFUSALS, SS_ERR_INVALID, SS_ERR_STATE

ACCEPTING = [n for n in dc.CASE_NAMES if dc.CASES[n].refuse is None]
REFUSING = [n for n in dc.CASE_NAMES if dc.CASES[n].refuse is not None]


def test_chunk_size_is_the_one_the_cases_aim_at():
    assert dc.PK_CHUNK == 2048 and (dc.S1, dc.S2, dc.S3) == (2048, 4096, 6144)


def test_case_list_covers_every_group_and_stays_small():
    assert len(dc.CASE_NAMES) == len(set(dc.CASE_NAMES)) == len(dc.CASES)
    assert {dc.CASES[n].group for n in dc.CASE_NAMES} == set(dc.GROUPS)
    for g in dc.GROUPS:
        if g != "refusals":
            assert sum(dc.CASES[n].score for n in dc.CASE_NAMES if dc.CASES[n].group == g) == 1, g      # one scored case per group
    for n in dc.CASE_NAMES:
        c = dc.CASES[n]
        assert len(c.table[1]) <= 3 * 2048 + 1 and c.n_terms <= 600 and c.n_docs <= 4400, n
        assert not (c.refuse and c.score), n
    assert {len(dc.CASES[n].table[1]) for n in dc.CASE_NAMES} >= {1, 2047, 2048, 2049, 6144, 6145}
    assert len(ACCEPTING) >= 45 and len(REFUSING) >= 15


@pytest.mark.parametrize("name", dc.CASE_NAMES)
def test_case_reaches_its_path(name):
    assert dc.reaches(dc.CASES[name])


@pytest.mark.parametrize("name", dc.CASE_NAMES)
def test_weights_and_positions_are_distinct(name):
    c = dc.CASES[name]
    w = np.concatenate([c.table[2]] + [d.add_w for d in c.deltas])
    assert len(np.unique(w)) == len(w)                                  # over the table and everything any delta brings
    if c.pos is not None:
        p = np.concatenate([c.pos[1]] + [d.add_pos for d in c.deltas if d.add_pos is not None])
        assert len(np.unique(p)) == len(p)
        assert len(np.unique(np.diff(c.pos[0].astype(np.int64)))) >= 3  # list lengths differ, zero among them
        assert (np.diff(c.pos[0].astype(np.int64)) == 0).any()


def ascending(tp, pd):
    tp = tp.astype(np.int64)
    first = np.zeros(len(pd), dtype=bool)
    first[tp[:-1][tp[:-1] < len(pd)]] = True
    return bool(np.all((np.diff(pd.astype(np.int64)) > 0) | first[1:])) if len(pd) > 1 else True


@pytest.mark.parametrize("name", ACCEPTING)
def test_accepting_case_gives_strictly_ascending_lists(name):
    c = dc.CASES[name]
    stages, reason = c.expected()
    assert reason is None and len(stages) == len(c.deltas) + 1
    for tp, pd, w, pp, pv, mag2, mag in stages:
        assert tp[0] == 0 and int(tp[-1]) == len(pd) == len(w) == len(pp) - 1 and np.all(np.diff(tp.astype(np.int64)) >= 0)
        assert ascending(tp, pd) and (len(pd) == 0 or int(pd.max()) < c.n_docs)
        assert int(pp[-1]) == len(pv) and np.all(np.diff(pp.astype(np.int64)) >= 0)
    assert not ascending(np.array([0, 2, 4], np.uint64), np.array([1, 1, 0, 5], np.uint32))       # the check can fail


@pytest.mark.parametrize("name", REFUSING)
def test_refusing_case_is_refused_for_its_reason(name):
    c = dc.CASES[name]
    stages, reason = c.expected()
    assert reason == c.refuse and len(stages) == len(c.deltas)         # every delta before the last is accepted
    assert REFUSALS[reason] == (SS_ERR_STATE if reason == "held" else SS_ERR_INVALID)
    if reason == "held":                                               # the delta itself is fine
        m = c.model()
        m.apply(c.deltas[-1])


def scratch_merge(n_terms, arrays, delta, positional):
    """The merge said once more, without rows: drop, append, sort by (term, doc).  arrays = (term_ptr, post_doc, post_w, pos_ptr, pos)."""
    tp, pd, w, pp, pv = arrays
    term = np.repeat(np.arange(n_terms, dtype=np.uint64), np.diff(tp.astype(np.int64)))
    key = (term << np.uint64(32)) | pd.astype(np.uint64)
    gone = np.isin(pd, delta.del_docs) | np.isin(key, (delta.del_term.astype(np.uint64) << np.uint64(32)) | delta.del_doc.astype(np.uint64))
    keep = np.flatnonzero(~gone)
    akey = (delta.add_term.astype(np.uint64) << np.uint64(32)) | delta.add_doc.astype(np.uint64)
    all_key = np.concatenate([key[keep], akey])
    all_w = np.concatenate([w[keep], delta.add_w])
    chunks = [pv[int(pp[i]):int(pp[i + 1])] for i in keep]
    if positional and delta.add_pos_ptr is not None:
        chunks += [delta.add_pos[int(delta.add_pos_ptr[j]):int(delta.add_pos_ptr[j + 1])] for j in range(len(akey))]
    else:
        chunks += [np.zeros(0, np.float32)] * len(akey)
    order = np.argsort(all_key, kind="stable")
    assert len(np.unique(all_key)) == len(all_key)
    new_tp = np.searchsorted(all_key[order] >> np.uint64(32), np.arange(n_terms + 1, dtype=np.uint64)).astype(np.uint64)
    chunks = [chunks[i] for i in order]
    new_pp = np.concatenate([[0], np.cumsum([len(x) for x in chunks])]).astype(np.uint64)
    new_pv = np.concatenate(chunks + [np.zeros(0, np.float32)]).astype(np.float32)
    return new_tp, (all_key[order] & np.uint64(0xFFFFFFFF)).astype(np.uint32), all_w[order].astype(np.float32), new_pp, new_pv


@pytest.mark.parametrize("name", ACCEPTING)
def test_model_agrees_with_a_from_scratch_flatten(name):
    c = dc.CASES[name]
    stages, _ = c.expected()
    cur = stages[0][:5]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(cur[:3], c.table))             # the model reads the table back as given
    if c.pos is not None:
        assert cur[3].tobytes() == c.pos[0].tobytes() and cur[4].tobytes() == c.pos[1].tobytes()
    else:
        assert not cur[3].any() and len(cur[4]) == 0
    for k, d in enumerate(c.deltas):
        cur = scratch_merge(c.n_terms, cur, d, c.pos is not None)
        for got, want, what in zip(cur, stages[k + 1][:5], ("term_ptr", "post_doc", "post_w", "pos_ptr", "pos")):
            assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (k, what)


@pytest.mark.parametrize("name", dc.CASE_NAMES)
def test_magnitudes_are_exact_in_any_order(name):
    """Every doc's float64 sum of float32 squares is exact whatever the order (all squares are multiples of one power of two and
    the sum of all of them stays below 2^53 of it), so the delta's own sums, a full pass and this bincount must give the same bits;
    the model's touched-docs-only update equals a sum over the whole table."""
    c = dc.CASES[name]
    stages, _ = c.expected()
    for k, (tp, pd, w, pp, pv, mag2, mag) in enumerate(stages):
        sq = (w * w).astype(np.float32)
        if len(sq):
            unit = max(Fraction(float(x)).denominator for x in sq)
            assert unit & (unit - 1) == 0
            per_doc = np.bincount(pd, weights=sq.astype(np.float64), minlength=c.n_docs)
            assert all(Fraction(float(x)) * unit < 2 ** 53 for x in per_doc)
            exact = [Fraction(0)] * c.n_docs
            for d_, x in zip(pd.tolist(), sq.tolist()):
                exact[d_] += Fraction(x)
            assert all(Fraction(float(per_doc[d_])) == exact[d_] for d_ in range(c.n_docs))
        else:
            per_doc = np.zeros(c.n_docs)
        if c.mag_valid:
            assert mag2.tobytes() == per_doc.astype(np.float64).tobytes() and mag.tobytes() == np.sqrt(per_doc).tobytes(), k
        else:
            assert not mag2.any() and not mag.any()


def test_the_model_refuses_and_accepts_what_the_header_says():
    """hand-made, so that the model is not only held against itself"""
    from tests.index_delta_model import Delta, Refused, TableModel
    tp, pd, w = np.array([0, 2, 2, 3], np.uint64), np.array([1, 4, 2], np.uint32), np.array([.5, .25, 2], np.float32)
    mk = lambda: TableModel(5, tp, pd, w, pos_ptr=np.array([0, 1, 1, 3], np.uint64), pos=np.array([7, 8, 9], np.float32), mag_valid=True)
    m = mk()
    assert m.mag2.tolist() == [0, .25, 4, 0, .0625] and m.mag.tolist() == [0, .5, 2, 0, .25]
    for delta, reason in ((Delta(del_docs=[5]), "del_docs_range"), (Delta(del_pairs=([3], [0])), "pair_range"), (Delta(del_pairs=([0], [5])), "pair_range"),
                          (Delta(add=([3], [0], [1])), "add_range"), (Delta(add=([0], [5], [1])), "add_range"),
                          (Delta(add=([1, 0, 1], [3, 3, 3], [1, 2, 3])), "add_twice"), (Delta(add=([0], [4], [1])), "add_exists"),
                          (Delta(add=([1], [0], [1]), add_pos=([1, 1], [])), "add_pos_ptr_start"),
                          (Delta(add=([1, 1], [0, 1], [1, 1]), add_pos=([0, 2, 1], [1, 2])), "add_pos_ptr_order")):
        with pytest.raises(Refused) as e:
            m.apply(delta)
        assert e.value.reason == reason and e.value.code == 1
        assert all(a.tobytes() == b.tobytes() for a, b in zip(m.flatten(), mk().flatten()))
    with pytest.raises(Refused) as e:
        m.apply(Delta(), held=True)
    assert e.value.code == 6
    # del_docs first, then pairs, then additions; a missing pair is ignored; positions follow
    m.apply(Delta(del_docs=[4, 4], del_pairs=([2, 1, 0], [2, 2, 3]), add=([2, 0, 1], [2, 4, 0], [3, 1, -1]), add_pos=([0, 0, 2, 2], [5, 6])))
    g_tp, g_pd, g_w, g_pp, g_pv = m.flatten()
    assert g_tp.tolist() == [0, 2, 3, 4] and g_pd.tolist() == [1, 4, 0, 2] and g_w.tolist() == [.5, 1, -1, 3]
    assert g_pp.tolist() == [0, 1, 3, 3, 3] and g_pv.tolist() == [7, 5, 6]
    assert m.mag2.tolist() == [1, .25, 9, 0, 1] and m.mag.tolist() == [1, .5, 3, 0, 1]
