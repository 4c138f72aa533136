"""GPU parity at the numeric edges of the top-k filter: clean inputs (tests/score_edge_inputs.py) whose impacts, coefficients,
priors and list lengths sit where the filter's float32 / fixed-point bounds and its threshold floor could drop a true winner.

For every case and k the hits of
  * k_score_slices alone (score.small = 0, score.wave = 0, small slices so that queries span several),
  * k_score_wave forced (score.small = 0, score.wave_min_list = 0, score.wave_slice_target = 1024) for k it takes,
  * the default routing, with host outputs and with device outputs,
  * a scorer created under score.exact_all = 1 (the filter off),
must equal the CPU oracle — same n_hits, same doc ids, title / body / pagerank / final bit-identical — and one another byte for
byte.  One masked and one constrained call per family (a 50 % random allow-list) go through the same comparison: a mask removes
the floor but keeps the filter.  No tolerance: bit-exact is this path's gate (tests/test_gpu_score.py) and the generator keeps
every float64 sum order-free.

First run on an MI355X: families B, C, D, E and the subnormal half of A passed as the library stood; the cases of family A with
title impacts beyond FLT_MAX / 1.31 failed in k_score_wave alone (smallest: A.title+140.body-155, k = 1, every query 0 rows
instead of 1) — the combined lists stepped the pre-scaled title impact two ulps past +Inf into a NaN, which the sketch counts as
one unit (fixed in k_merge_lists).
"""
import numpy as np
import pytest

from spaghettisearch_amd import engine
from tests import score_edge_inputs as edge

pytestmark = pytest.mark.gpu

WAVE_MAX_K = 128          # k_score_wave's candidate buffer holds 2k entries of 256; the host sends larger k to k_score_slices


def assert_same_hits(hits, n_hits, ref, ref_n, exact=True):
    assert n_hits.tolist() == ref_n.tolist()
    for q in range(len(n_hits)):
        n = int(n_hits[q])
        assert hits["doc"][q, :n].tolist() == ref["doc"][q, :n].tolist(), f"query {q}"
        for f in ("title", "body", "pagerank", "final"):
            a, b = hits[f][q, :n], ref[f][q, :n]
            if exact:
                assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (q, f, a[:5], b[:5])
            else:
                np.testing.assert_allclose(a, b, rtol=1e-6)


# ---- reference --------------------------------------------------------------------------------------------------------------------

def restrict_table(table, allowed, pos=None):
    """(term_ptr, post_doc, post_w) without the postings of disallowed docs; pos = (pos_ptr, pos) likewise."""
    ptr, doc, w = (np.asarray(a) for a in table)
    ptr = ptr.astype(np.int64)
    keep = allowed[doc.astype(np.int64)]
    term = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    cnt = np.bincount(term[keep], minlength=len(ptr) - 1)
    out = (np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64), doc[keep].astype(np.uint32), w[keep].astype(np.float32))
    if pos is None:
        return out, None
    pp, pv = np.asarray(pos[0]).astype(np.int64), np.asarray(pos[1])
    plen = np.diff(pp)[keep]
    return out, (np.concatenate([[0], np.cumsum(plen)]).astype(np.uint64), pv[np.repeat(keep, np.diff(pp))].astype(np.float32))


def oracle_hits(oracle, c, k, allowed=None):
    """The oracle's rows of case c at k.  allowed: per query a bool [n_docs] allow-list or None (the query may return any doc):
    the oracle then runs over the tables without the postings of the other docs."""
    if allowed is None:
        allowed = [None] * c.n_q
    hits = np.zeros((c.n_q, k), dtype=engine.HIT_DTYPE)
    n_hits = np.zeros(c.n_q, dtype=np.int32)
    groups = {}
    for q, a in enumerate(allowed):
        groups.setdefault(None if a is None else a.tobytes(), []).append(q)
    for qs in groups.values():
        a = allowed[qs[0]]
        title, body, tpos, bpos = c.title, c.body, None, None
        if c.positions is not None:
            tpos, bpos = c.positions
        if a is not None:
            title, tpos = restrict_table(c.title, a, tpos)
            body, bpos = restrict_table(c.body, a, bpos)
        if c.phrases is None:
            idx = np.array(qs)
            qp = np.concatenate([[0], np.cumsum([len(c.query(q)) for q in qs])]).astype(np.uint32)
            qt = np.concatenate([c.query(q) for q in qs]).astype(np.uint32)
            kw = {"query_len": c.query_len[idx]}
            if c.prior is not None:
                kw.update(prior=c.prior, topic_probs=c.topic_probs[idx])
            r, rn = oracle.score_topk_batch(c.n_docs, title, body, c.mag_t, c.mag_b, qp, qt, k, **kw)
            hits[idx], n_hits[idx] = r, rn
            continue
        n_terms = len(c.body[0]) - 1
        for q in qs:
            ph, extra = c.phrase(q), None
            if len(ph):
                extra = (np.zeros(0, np.uint32), np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.uint8))
                if all(int(t) < n_terms for t in ph):
                    extra = oracle.phrase(title, body, tpos, bpos, ph)
            r, _ = oracle.score_topk(c.n_docs, title, body, c.mag_t, c.mag_b, c.query(q), k, query_len=int(c.query_len[q]), extra=extra)
            hits[q, :len(r)], n_hits[q] = r, len(r)
    return hits, n_hits


def contains(c, t):
    """bool [n_docs]: the docs with a title or body posting of term t."""
    out = np.zeros(c.n_docs, dtype=bool)
    for ptr, doc, _ in (c.title, c.body):
        out[doc[int(ptr[t]):int(ptr[t + 1])].astype(np.int64)] = True
    return out


# ---- the library under test ---------------------------------------------------------------------------------------------------------

class Scorers:
    """The case's tables on the device twice: one scorer as the library makes it (filter on), one made under score.exact_all."""

    def __init__(self, ctx, c):
        self.ctx, self.c, self.open = ctx, c, []
        self.on = self._make()
        with ctx.options(score__exact_all=1):
            self.off = self._make()

    def _make(self):
        c = self.c
        ti = engine.InvertedIndex(self.ctx, c.n_docs, *c.title)
        self.open.append(ti)
        bi = engine.InvertedIndex(self.ctx, c.n_docs, *c.body)
        self.open.append(bi)
        ti.set_weighted(c.mag_t)
        bi.set_weighted(c.mag_b)
        if c.positions is not None:
            ti.set_positions(*c.positions[0])
            bi.set_positions(*c.positions[1])
        sc = engine.Scorer(self.ctx, ti, bi)
        self.open.append(sc)
        if c.prior is not None:
            sc.set_prior(np.ascontiguousarray(c.prior.T))
        return sc

    def close(self):
        for x in [o for o in self.open if isinstance(o, engine.Scorer)] + [o for o in self.open if not isinstance(o, engine.Scorer)]:
            x.close()


def run(sc, c, k, device_out=False):
    """One plain call of case c (the phrase entry point for the phrase family) -> (hits [n_q][k], n_hits) on the host."""
    out = None
    if device_out:
        import torch
        dev = torch.device("cuda", 0)
        out = (torch.zeros(c.n_q * k * engine.HIT_DTYPE.itemsize, dtype=torch.uint8, device=dev), torch.zeros(c.n_q, dtype=torch.int32, device=dev))
    if c.phrases is not None:
        if out is None:
            return sc.score_topk_phrase(c.q_ptr, c.q_terms, c.phrases[0], c.phrases[1], k, query_len=c.query_len)
        sc.score_topk_masked(c.q_ptr, c.q_terms, None, k, p_ptr=c.phrases[0], p_terms=c.phrases[1], query_len=c.query_len, out=out)
    else:
        r = sc.score_topk(c.q_ptr, c.q_terms, k, query_len=c.query_len, topic_probs=c.topic_probs, out=out)
        if out is None:
            return r
    return out[0].cpu().numpy().view(engine.HIT_DTYPE).reshape(c.n_q, k), out[1].cpu().numpy()


SLICES = dict(score__small=0, score__wave=0, score__slice_target=2048)
WAVE = dict(score__small=0, score__wave_min_list=0, score__wave_slice_target=1024, score__wave_max_terms=12)
FILTER_OFF = dict(score__small=0, score__slice_target=2048)


def compare(failures, label, got, ref):
    try:
        assert_same_hits(got[0], got[1], ref[0], ref[1], exact=True)
    except AssertionError as exc:
        failures.append(f"{label}: {str(exc)[:300]}")


@pytest.mark.parametrize("name", edge.CASE_NAMES)
def test_filter_edges_match_oracle(ss_ctx, oracle, name):
    c = edge.get_case(name)
    s = Scorers(ss_ctx, c)
    failures = []
    try:
        for k in c.ks:
            ref = oracle_hits(oracle, c, k)
            runs = {}
            with ss_ctx.options(**SLICES):
                runs["slices"] = run(s.on, c, k)
            if k <= WAVE_MAX_K and c.phrases is None:
                with ss_ctx.options(**WAVE):
                    runs["wave"] = run(s.on, c, k)
            runs["default"] = run(s.on, c, k)
            runs["default, device outputs"] = run(s.on, c, k, device_out=True)
            with ss_ctx.options(**FILTER_OFF):
                runs["filter off"] = run(s.off, c, k)
            for mode, got in runs.items():
                compare(failures, f"{name} k={k} {mode}", got, ref)
            off = runs["filter off"]
            for mode, got in runs.items():
                if got[0].tobytes() != off[0].tobytes() or got[1].tolist() != off[1].tolist():
                    failures.append(f"{name} k={k} {mode}: bytes differ from the filter-off scorer's")
    finally:
        s.close()
    assert not failures, "\n".join(failures[:40]) + f"\n({len(failures)} in all)"


@pytest.mark.parametrize("name", edge.MASKED_NAMES)
def test_masked_and_constrained_calls_match_oracle(ss_ctx, oracle, name):
    """score_topk_masked and score_topk_constrained over a 50 % random allow-list (three queries in four; the fourth is free and
    keeps its floor), the constrained call with a required and, every third query, an excluded term on top."""
    c = edge.get_case(name)
    rng = np.random.default_rng(len(name))
    allow = rng.random(c.n_docs) < 0.5
    mask_id = np.where(np.arange(c.n_q) % 4 == 3, -1, 0).astype(np.int32)
    n_terms = len(c.body[0]) - 1
    by_len = np.argsort(-(np.diff(c.body[0].astype(np.int64)) + np.diff(c.title[0].astype(np.int64))))
    req = [[int(by_len[q % 4])] if q % 2 == 0 else [] for q in range(c.n_q)]
    exc = [[int(by_len[4 + q % 3])] if q % 3 == 0 else [] for q in range(c.n_q)]
    assert max(max(x, default=0) for x in req + exc) < n_terms
    masked_sets = [allow if m >= 0 else None for m in mask_id]
    constrained_sets = []
    for q in range(c.n_q):
        a = allow.copy() if mask_id[q] >= 0 else np.ones(c.n_docs, dtype=bool)
        for t in req[q]:
            a &= contains(c, t)
        for t in exc[q]:
            a &= ~contains(c, t)
        constrained_sets.append(a if (mask_id[q] >= 0 or req[q] or exc[q]) else None)

    def pairs(lists):
        return (np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint32), np.array([t for x in lists for t in x], dtype=np.uint32))
    ph = {} if c.phrases is None else {"p_ptr": c.phrases[0], "p_terms": c.phrases[1]}
    s = Scorers(ss_ctx, c)
    failures = []
    try:
        for sc in (s.on, s.off):
            sc.set_doc_masks(engine.pack_doc_masks(allow[None, :], c.n_docs))
        for k in (c.ks[1], c.ks[-2]):
            ref_m = oracle_hits(oracle, c, k, masked_sets)
            ref_c = oracle_hits(oracle, c, k, constrained_sets)
            for label, sc, opts in (("filter on", s.on, dict(score__small=0, score__wave_min_list=0, score__slice_target=2048)),
                                    ("default", s.on, {}), ("filter off", s.off, FILTER_OFF)):
                with ss_ctx.options(**opts):
                    got_m = sc.score_topk_masked(c.q_ptr, c.q_terms, mask_id, k, query_len=c.query_len, topic_probs=c.topic_probs, **ph)
                    got_c = sc.score_topk_constrained(c.q_ptr, c.q_terms, k, req=pairs(req), exc=pairs(exc), mask_id=mask_id,
                                                      query_len=c.query_len, topic_probs=c.topic_probs, **ph)
                compare(failures, f"{name} k={k} masked, {label}", got_m, ref_m)
                compare(failures, f"{name} k={k} constrained, {label}", got_c, ref_c)
    finally:
        s.close()
    assert not failures, "\n".join(failures[:40]) + f"\n({len(failures)} in all)"
