"""CPU side of the filter-edge suite (tests/score_edge_inputs.py): every case meets the generator's three conditions (clean by
the library's rule, order-free float64 sums, a live cut), and the C oracle equals its numpy twin BIT FOR BIT on it — +Inf and
subnormal FinalRanks, whole tiers of ties in ascending doc id, rows filled with FinalRank-0 documents included.  That is what
can be checked without a GPU, and it raises trust in the oracle exactly where tests/test_gpu_score_filter_edges.py leans on it.

The phrase family has no numpy twin (oracle_np has no phrase part): its cases are checked for the conditions and for real
phrase matches through orc_phrase, as tests/test_gpu_phrase.py uses it.

The last two tests pin the arithmetic that motivated the suite: a threshold floor taken from the EXACT k'-th largest float32
impact would exceed the true FinalRank for subnormal impacts and for impacts beyond FLT_MAX — and the bound the library
really stores (k_kth_impact: a histogram edge in [2^-8, 1), 0 below it) does not.
"""
import numpy as np
import pytest

from oracle import oracle_np
from tests import score_edge_inputs as edge


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def phrase_extra(oracle, c, q):
    ph = c.phrase(q)
    if len(ph) == 0:
        return None
    if not all(int(t) < len(c.body[0]) - 1 for t in ph):
        return (np.zeros(0, np.uint32), np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.uint8))
    return oracle.phrase(c.title, c.body, c.positions[0], c.positions[1], ph)


def oracle_candidates(oracle, c):
    """Candidate documents per query as the C oracle counts them."""
    out = np.zeros(c.n_q, dtype=np.int64)
    for q in range(c.n_q):
        kw = {}
        if c.prior is not None:
            kw = {"prior": c.prior, "topic_probs": c.topic_probs[q]}
        _, n_cand = oracle.score_topk(c.n_docs, c.title, c.body, c.mag_t, c.mag_b, c.query(q), 1, query_len=int(c.query_len[q]),
                                      extra=phrase_extra(oracle, c, q) if c.phrases is not None else None, **kw)
        out[q] = n_cand
    return out


@pytest.mark.parametrize("name", edge.CASE_NAMES)
def test_case_meets_conditions_and_oracles_agree(oracle, name):
    c = edge.get_case(name)                       # (check_case has asserted "clean" and "exact")
    n_cand = oracle_candidates(oracle, c)
    live = np.array([any(n > k for k in c.ks) for n in n_cand])
    print(f"\n{name}: docs {c.n_docs} queries {c.n_q} k {c.ks}  clean: yes  weight spread 2^{c.figures['spread_log2']:.0f} (<= 2^28)  "
          f"impacts 2^{c.figures['impact_log2_min']:.1f} .. 2^{c.figures['impact_log2_max']:.1f}  "
          f"candidates {int(n_cand.min())} .. {int(n_cand.max())}  live cut: {int(live.sum())}/{c.n_q} queries")
    assert live.mean() >= 0.75, (name, live.mean())
    if c.phrases is not None:
        n_match = sum(len(x[0]) for x in (phrase_extra(oracle, c, q) for q in range(c.n_q)) if x is not None)
        assert n_match > 20, n_match              # the quoted phrases do match documents
        return
    assert np.array_equal(n_cand, edge.candidate_counts(c))
    k_max = max(c.ks)
    twin = []
    for q in range(c.n_q):
        kw = {}
        if c.prior is not None:
            kw = {"prior": c.prior, "topic_probs": c.topic_probs[q]}
        twin.append(oracle_np.score_topk(c.n_docs, c.title, c.body, c.mag_t, c.mag_b, c.query(q), k_max,
                                         query_len=int(c.query_len[q]), **kw))
    n_special = 0
    for k in c.ks:
        ref, ref_n = oracle.score_topk_batch(c.n_docs, c.title, c.body, c.mag_t, c.mag_b, c.q_ptr, c.q_terms, k, **c.oracle_kw())
        for q in range(c.n_q):
            docs, T, B, sqd, final = twin[q]
            n = min(k, len(docs))
            assert int(ref_n[q]) == n == min(k, int(n_cand[q])), (name, k, q)
            assert ref["doc"][q, :n].tolist() == docs[:n].tolist(), (name, k, q)
            for f, v in (("title", T), ("body", B), ("pagerank", sqd), ("final", final)):
                assert np.array_equal(bits(ref[f][q, :n]), bits(v[:n])), (name, k, q, f)
            fin = ref["final"][q, :n]
            assert not np.isnan(fin).any()                                    # clean inputs cannot give NaN
            assert (fin[1:] <= fin[:-1]).all()                                # descending, and ties by ascending doc id
            tie = fin[1:] == fin[:-1]
            assert (np.diff(ref["doc"][q, :n].astype(np.int64))[tie] > 0).all()
            n_special += int(np.isinf(fin).sum()) + int(((fin > 0) & (fin < 2.0 ** -126)).sum()) + int(tie.sum())
    if name in ("A.both-155", "A.both+140", "A.perdoc", "D.sqd_overflow", "D.absorbed_ties", "B.floor"):
        assert n_special > 0, name                # the edge the case is named for shows in the oracle's rows


# ---- the arithmetic behind the suite ---------------------------------------------------------------------------------------------

def f32_round_up(x):
    """float64 -> the smallest float32 >= x (__double2float_ru)."""
    with np.errstate(over="ignore"):
        y = np.float32(x)
    return y if np.float64(y) >= x else np.nextafter(y, np.float32(np.inf))


def f32_round_down(x):
    """float64 -> the largest float32 <= x (__double2float_rd)."""
    with np.errstate(over="ignore"):
        y = np.float32(x)
    return y if np.float64(y) <= x else np.nextafter(y, np.float32(-np.inf))


def stored_kth_bound(impacts_f32, kp):
    """The k'-th largest impact of a list as the library stores it (k_kth_impact): each impact, stepped down by 2^-21 relative,
    falls into one of 4096 bins over [2^-8, 1) (9 mantissa bits per binade, everything at and above 1 in the top bin, everything
    below 2^-8 in bin 0 whose edge is 0); the bound is the lower edge of the bin at which the count from the top reaches k'."""
    b0 = np.uint32(0x3B800000)
    with np.errstate(invalid="ignore", over="ignore"):
        lb = (np.asarray(impacts_f32, dtype=np.float32) * np.float32(1.0 - 2.0 ** -21)).astype(np.float32)
    lb = lb[lb > 0]
    xb = lb.view(np.uint32)
    b = np.where(xb >= b0, np.minimum((xb.astype(np.int64) - int(b0)) >> 14, 4095), 0)
    if len(b) < kp:
        return np.float32(0.0)
    edge_bin = int(np.sort(b)[::-1][kp - 1])
    return np.float32(0.0) if edge_bin == 0 else np.array([int(b0) + (edge_bin << 14)], dtype=np.uint32).view(np.float32)[0]


def floor_of(kth, field_coef=29.0, mult=1, query_len=1):
    """score.hip / score_wave.hip: share * (1 - 2^-12) * kth rounded down to float32."""
    share = field_coef * float(mult) / np.sqrt(np.float64(query_len))
    return f32_round_down(share * (1.0 - 2.0 ** -12) * np.float64(kth))


def one_list_final(oracle, w, mag, n=4):
    """FinalRank of the documents of a one-term body table of n equal postings, query_len = 1."""
    body = (np.array([0, n], np.uint64), np.arange(n, dtype=np.uint32), np.full(n, w, np.float32))
    title = (np.array([0, 0], np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.float32))
    hits, n_hits = oracle.score_topk_batch(n, title, body, np.ones(n), np.full(n, mag), np.array([0, 1], np.uint32), np.array([0], np.uint32), n)
    assert int(n_hits[0]) == n and len(set(hits["final"][0].tolist())) == 1
    return float(hits["final"][0, 0])


def test_worked_example_subnormal_impact(oracle):
    w, mag = np.float32(1e-3), 1e40
    imp = f32_round_up(np.float64(w) / mag)                      # impact_of: w / mag rounded UP to float32
    unit = 2.0 ** -149
    assert np.float64(w) / mag / unit == pytest.approx(71.36, abs=0.01) and float(imp) / unit == 72.0
    final = one_list_final(oracle, w, mag)
    assert final == pytest.approx(2.9000e-42, rel=1e-4)
    # a floor from the exact k'-th largest stored impact would lie ABOVE the truth: 2.9245e-42 > 2.9000e-42 ...
    unsafe = float(floor_of(imp))
    assert unsafe == pytest.approx(2.9245e-42, rel=1e-4) and unsafe > final
    # ... but the stored bound of an impact below 2^-8 is 0, and a list whose bound is 0 gives no floor
    assert stored_kth_bound(np.full(4, imp), 4) == 0.0
    # the smallest impact that has a bound at all: 2^-8, a normal float32 whose round-up error is far inside the 2^-12 margin
    kth = stored_kth_bound(np.full(4, np.float32(2.0 ** -8 * 1.01)), 4)
    assert 2.0 ** -8 <= float(kth) <= 2.0 ** -8 * 1.01
    assert float(floor_of(kth)) <= one_list_final(oracle, np.float32(2.0 ** -8 * 1.01), 1.0)


def test_worked_example_impact_beyond_flt_max(oracle):
    w, mag = np.float32(1e20), 1e-30
    imp = f32_round_up(np.float64(w) / mag)
    assert np.isinf(imp)                                          # impact_of rounds up to +Inf
    final = one_list_final(oracle, w, mag)
    assert np.isfinite(final) and final == pytest.approx(2.9e51, rel=1e-3)
    assert np.isinf(floor_of(imp)) and float(floor_of(imp)) > final      # a floor from the exact k'-th largest impact: +Inf
    kth = stored_kth_bound(np.full(4, imp), 4)                    # the stored bound: the top bin's edge, just below 1
    assert 0.99 < float(kth) < 1.0
    assert float(floor_of(kth)) < 29.0 < final
