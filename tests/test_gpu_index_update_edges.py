"""GPU: ss_index_apply_delta(_pos) on the constructed cases of tests/index_delta_cases.py, byte for byte against
tests/index_delta_model.py (tests/test_index_delta_cases_cpu.py shows on the CPU that every case stands on the path it names).

Per case: create the table (positions, magnitudes where the case has them), apply the delta(s), and after each one read back
term_ptr, post_doc, post_w, pos_ptr, pos and the magnitude of EVERY doc and compare their bytes with the model's.  Where the
magnitudes are resident they are also held against ss_index_refresh_magnitudes on a fresh index made of the model's merged table
(the cases' sums are exact in any order, so a full pass has no other bits to give).  A refusing case returns its code and leaves
every one of those arrays as it was.  One case per group also scores on the updated table and on a fresh copy of the model's.
(The squared magnitudes have no read call of their own: they show as mag = sqrt(mag2).)
"""
import numpy as np
import pytest

from spaghettisearch_amd import _lib
from tests import index_delta_cases as dc
from tests.index_delta_model import REFUSALS

pytestmark = pytest.mark.gpu

WHAT = ("term_ptr", "post_doc", "post_w", "pos_ptr", "pos", "mag")


def make_index(ctx, n_docs, tp, pd, w, pos=None, magnitudes=False):
    from spaghettisearch_amd import engine
    idx = engine.InvertedIndex(ctx, n_docs, tp, pd, w)
    try:
        if pos is not None:
            idx.set_positions(pos[0], pos[1])
        if magnitudes:
            idx.refresh_magnitudes()
    except Exception:
        idx.close()
        raise
    return idx


def read_all(idx, positional):
    """what WHAT names, as the table stands"""
    tp, pd, w = idx.read()
    pp, pv = idx.read_positions() if positional else (np.zeros(len(pd) + 1, np.uint64), np.zeros(0, np.float32))
    mag = idx.read_magnitudes(np.arange(idx.n_docs, dtype=np.uint32))
    return tp, pd, w, pp, pv, mag


def assert_same_bytes(got, want, where):
    for g, e, what in zip(got, want, WHAT):
        assert g.dtype == e.dtype and g.shape == e.shape, (where, what, g.shape, e.shape)
        if g.tobytes() != e.tobytes():
            bad = np.flatnonzero(g.view(f"u{g.itemsize}") != e.view(f"u{e.itemsize}"))
            raise AssertionError(f"{where}: {what} differs at {bad[:8].tolist()} ({len(bad)} entries): got {g[bad[:8]].tolist()}, model {e[bad[:8]].tolist()}")


def apply(idx, d):
    idx.apply_delta(del_docs=d.del_docs, del_pairs=(d.del_term, d.del_doc), add=(d.add_term, d.add_doc, d.add_w),
                    add_pos=None if d.add_pos_ptr is None else (d.add_pos_ptr, d.add_pos))


def queries_over(case):
    """single terms and pairs of the terms the deltas touch (and their neighbours)"""
    terms = set()
    tp, pd, _ = case.table
    term_of = dc.term_of(case)
    for d in case.deltas:
        terms |= {int(t) for t in np.concatenate([d.del_term, d.add_term]) if t < case.n_terms}
        terms |= set(term_of[np.isin(pd, d.del_docs)].tolist())
    terms = sorted(terms)[:24]
    qs = [[t] for t in terms] + [[a, b] for a, b in zip(terms, terms[1:])] + [[min(t + 1, case.n_terms - 1), t] for t in terms[:4] if t + 1 < case.n_terms]
    q_ptr = np.concatenate([[0], np.cumsum([len(q) for q in qs])]).astype(np.uint32)
    return q_ptr, np.array([t for q in qs for t in q], dtype=np.uint32)


def hits_on(ctx, title, body, q_ptr, q_terms):
    from spaghettisearch_amd import engine
    sc = engine.Scorer(ctx, title, body)
    try:
        hits, n_hits = sc.score_topk(q_ptr, q_terms, 10)
    finally:
        sc.close()
    return hits, n_hits


@pytest.mark.parametrize("name", dc.CASE_NAMES)
def test_delta_case(ss_ctx, name):
    from spaghettisearch_amd import engine
    case = dc.CASES[name]
    stages, reason = case.expected()
    assert reason == case.refuse
    positional = case.pos is not None
    model_of = lambda st: st[:5] + (st[6],)
    idx = make_index(ss_ctx, case.n_docs, *case.table, pos=case.pos, magnitudes=case.mag_valid)
    others = []
    try:
        assert_same_bytes(read_all(idx, positional), model_of(stages[0]), "before any delta")
        for k, d in enumerate(case.deltas):
            where = f"delta {k}"
            if k == len(case.deltas) - 1 and reason is not None:
                before = read_all(idx, positional)
                holder = None
                if case.held:
                    others.append(make_index(ss_ctx, case.n_docs, *case.table, magnitudes=True))
                    holder = engine.Scorer(ss_ctx, others[-1], idx)
                try:
                    with pytest.raises(_lib.SpaghettiError) as e:
                        apply(idx, d)
                finally:
                    if holder is not None:
                        holder.close()
                assert e.value.code == REFUSALS[reason]
                assert_same_bytes(read_all(idx, positional), before, "after the refusal")
                assert_same_bytes(before, model_of(stages[-1]), "after the refusal (model)")
                continue
            apply(idx, d)
            st = stages[k + 1]
            assert idx.n_post == len(st[1])
            assert_same_bytes(read_all(idx, positional), model_of(st), where)
            if case.mag_valid:                                         # a full pass over a fresh copy of the model's table: the same bits
                fresh = make_index(ss_ctx, case.n_docs, st[0], st[1], st[2])
                try:
                    full = fresh.refresh_magnitudes()
                finally:
                    fresh.close()
                assert full.tobytes() == st[6].tobytes(), where
        if case.score:
            st = stages[-1]
            if not case.mag_valid:
                idx.refresh_magnitudes()
            others.append(make_index(ss_ctx, case.n_docs, *case.table, magnitudes=True))        # the title table: the case's, before the deltas
            others.append(make_index(ss_ctx, case.n_docs, st[0], st[1], st[2], magnitudes=True))
            q_ptr, q_terms = queries_over(case)
            assert len(q_terms) >= 8
            got, got_n = hits_on(ss_ctx, others[0], idx, q_ptr, q_terms)
            want, want_n = hits_on(ss_ctx, others[0], others[1], q_ptr, q_terms)
            assert got_n.tobytes() == want_n.tobytes() and got.tobytes() == want.tobytes()
            assert int(got_n.sum()) > 0
    finally:
        for o in others:
            o.close()
        idx.close()
