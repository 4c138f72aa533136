"""Generators of CLEAN scoring inputs at the numeric edges of the top-k filter (k_score_slices / k_score_wave).

The scorer drops postings whose float32 / fixed-point upper bound of FinalRank lies below a running threshold, and starts
that threshold from a floor taken from a list's k'-th largest impact.  It does so only for inputs it calls clean; this
module builds inputs that ARE clean by the library's own rule and sit where that arithmetic is least comfortable: impacts
w / magnitude far inside the float32 subnormals and beyond FLT_MAX, lists of exactly k' postings, coefficient spread and
clamp saturation, priors that swamp or vanish beside the term part, whole tiers of equal FinalRank, phrase records.

Every case is checked with numpy before it is handed out (`check_case`):

  clean      weights >= 0 and finite; magnitude > 0 and finite wherever a weight is non-zero; prior >= 0 and finite;
             topic probabilities >= 0 and finite; query_len >= 1.
  exact      within one document and one field the non-zero float32 weights span at most 28 binary orders (README: then
             float64 sums do not depend on their order).  The tables here are far tighter: weights are tf = c / m with
             c <= m <= 16 (four binary orders), a query adds at most 64 * 2 + 16 of them with multiplicities up to 64:
             24 + 4 + 14 bits < 53, every partial sum is exact.  The wide ranges come from the magnitudes.
  live cut   candidate counts (docs with a posting of a query term) are what the CPU test holds against the k list.

Used by tests/test_score_edge_inputs_cpu.py (oracle vs its numpy twin) and tests/test_gpu_score_filter_edges.py.
"""
from __future__ import annotations

import numpy as np

from spaghettisearch_amd import synth

K_ALL = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 512, 513, 1024)
MAX_SPREAD_LOG2 = 28
INT32_MAX = 2 ** 31 - 1


class EdgeCase:
    """One named case.  prior is node-major [n_docs][K] float64 (the oracle's layout; the scorer takes its transpose),
    topic_probs [n_q][K]; both None without a blend.  positions = ((t_pos_ptr, t_pos), (b_pos_ptr, b_pos)) and phrases =
    (p_ptr, p_terms) only in the phrase family.  `masked` marks the family's case for the masked / constrained calls."""

    def __init__(self, name, n_docs, title, body, mag_t, mag_b, q_ptr, q_terms, ks, query_len=None, prior=None, topic_probs=None,
                 positions=None, phrases=None, masked=False):
        self.name, self.family = name, name[0]
        self.n_docs = int(n_docs)
        self.title = tuple(np.ascontiguousarray(a, dtype=d) for a, d in zip(title, (np.uint64, np.uint32, np.float32)))
        self.body = tuple(np.ascontiguousarray(a, dtype=d) for a, d in zip(body, (np.uint64, np.uint32, np.float32)))
        self.mag_t = np.ascontiguousarray(mag_t, dtype=np.float64)
        self.mag_b = np.ascontiguousarray(mag_b, dtype=np.float64)
        self.q_ptr = np.ascontiguousarray(q_ptr, dtype=np.uint32)
        self.q_terms = np.ascontiguousarray(q_terms, dtype=np.uint32)
        self.ks = tuple(ks)
        n_q = len(self.q_ptr) - 1
        if query_len is None:
            query_len = np.diff(self.q_ptr.astype(np.int64))
            if phrases is not None:
                query_len = query_len + np.diff(np.asarray(phrases[0]).astype(np.int64))
        self.query_len = np.ascontiguousarray(query_len, dtype=np.int32)
        self.prior = None if prior is None else np.ascontiguousarray(prior, dtype=np.float64)
        self.topic_probs = None if topic_probs is None else np.ascontiguousarray(topic_probs, dtype=np.float64)
        self.positions, self.phrases, self.masked = positions, phrases, masked
        assert len(self.query_len) == n_q

    @property
    def n_q(self):
        return len(self.q_ptr) - 1

    def as_tuple(self):
        return (self.n_docs, self.title, self.body, self.mag_t, self.mag_b, self.q_ptr, self.q_terms, self.ks, self.query_len,
                self.prior, self.topic_probs)

    def query(self, q):
        return self.q_terms[int(self.q_ptr[q]):int(self.q_ptr[q + 1])]

    def phrase(self, q):
        if self.phrases is None:
            return np.zeros(0, np.uint32)
        return np.asarray(self.phrases[1])[int(self.phrases[0][q]):int(self.phrases[0][q + 1])]

    def oracle_kw(self):
        kw = {"query_len": self.query_len}
        if self.prior is not None:
            kw.update(prior=self.prior, topic_probs=self.topic_probs)
        return kw


# ---- the three conditions ----------------------------------------------------------------------------------------------------

def weight_spread_log2(n_docs, table):
    """Largest log2(max / min) of the non-zero weights of one document in this table (0 for an empty table)."""
    _, doc, w = table
    nz = w != 0
    if not nz.any():
        return 0.0
    d = doc[nz].astype(np.int64)
    lw = np.log2(w[nz].astype(np.float64))
    hi = np.full(n_docs, -np.inf)
    lo = np.full(n_docs, np.inf)
    np.maximum.at(hi, d, lw)
    np.minimum.at(lo, d, lw)
    seen = np.isfinite(hi)
    return float((hi[seen] - lo[seen]).max())


def check_case(c):
    """Assert the generator's conditions on one case; -> dict of the figures (for the test's report)."""
    n_terms = len(c.body[0]) - 1
    assert len(c.title[0]) - 1 == n_terms, c.name
    spread = 0.0
    for (ptr, doc, w), mag in ((c.title, c.mag_t), (c.body, c.mag_b)):
        assert int(ptr[0]) == 0 and int(ptr[-1]) == len(doc) == len(w), c.name
        assert (np.diff(ptr.astype(np.int64)) >= 0).all(), c.name
        assert len(doc) == 0 or int(doc.max()) < c.n_docs, c.name
        for t in range(n_terms):                            # strictly ascending docs inside a list
            d = doc[int(ptr[t]):int(ptr[t + 1])].astype(np.int64)
            assert (np.diff(d) > 0).all(), (c.name, t)
        assert np.isfinite(w).all() and (w >= 0).all(), c.name                          # clean: weights
        m = mag[doc[w != 0].astype(np.int64)]
        assert np.isfinite(m).all() and (m > 0).all(), c.name                           # clean: magnitudes under a non-zero weight
        assert len(mag) == c.n_docs and not np.isnan(mag).any(), c.name
        spread = max(spread, weight_spread_log2(c.n_docs, (ptr, doc, w)))
    assert spread <= MAX_SPREAD_LOG2, (c.name, spread)                                  # exact: order-free float64 sums
    assert (c.query_len >= 1).all(), c.name                                             # clean: query length
    assert (np.diff(c.q_ptr.astype(np.int64)) >= 0).all() and int(c.q_ptr[-1]) == len(c.q_terms), c.name
    if c.prior is not None:
        assert c.prior.shape[0] == c.n_docs and c.topic_probs.shape == (c.n_q, c.prior.shape[1]), c.name
        assert np.isfinite(c.prior).all() and (c.prior >= 0).all(), c.name              # clean: prior
        assert np.isfinite(c.topic_probs).all() and (c.topic_probs >= 0).all(), c.name  # clean: probabilities
    else:
        assert c.topic_probs is None, c.name
    assert all(1 <= k <= 1024 for k in c.ks) and set(c.ks) <= set(K_ALL), c.name
    imp = []
    for (ptr, doc, w), mag in ((c.title, c.mag_t), (c.body, c.mag_b)):
        nz = w != 0
        if nz.any():
            imp.append(w[nz].astype(np.float64) / mag[doc[nz].astype(np.int64)])
    imp = np.concatenate(imp) if imp else np.ones(1)
    with np.errstate(divide="ignore"):
        return {"spread_log2": spread, "impact_log2_min": float(np.log2(imp.min())), "impact_log2_max": float(np.log2(imp.max()))}


def candidate_counts(c):
    """Docs with a title or body posting of a known query term, per query (phrase matches are a subset of them only when the
    phrase's terms are query terms, so phrase cases are counted by the oracle itself in the CPU test)."""
    n_terms = len(c.body[0]) - 1
    out = np.zeros(c.n_q, dtype=np.int64)
    for q in range(c.n_q):
        seen = np.zeros(c.n_docs, dtype=bool)
        for t in set(int(x) for x in c.query(q)):
            if t < n_terms:
                for ptr, doc, _ in (c.title, c.body):
                    seen[doc[int(ptr[t]):int(ptr[t + 1])].astype(np.int64)] = True
        out[q] = int(seen.sum())
    return out


# ---- building blocks ---------------------------------------------------------------------------------------------------------

def _table(lists, weights):
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
    doc = np.concatenate(lists).astype(np.uint32) if lists else np.zeros(0, np.uint32)
    w = np.concatenate(weights).astype(np.float32) if weights else np.zeros(0, np.float32)
    return ptr, doc, w


def _l2(n_docs, table):
    """sqrt of a doc's summed float32 squares (the index's magnitude); 1 for a doc without postings."""
    _, doc, w = table
    sq = (w * w).astype(np.float32).astype(np.float64)
    m = np.sqrt(np.bincount(doc.astype(np.int64), weights=sq, minlength=n_docs))
    m[m == 0] = 1.0
    return m


def _pack(queries):
    q_ptr = np.concatenate([[0], np.cumsum([len(x) for x in queries])]).astype(np.uint32)
    q_terms = np.array([t for x in queries for t in x], dtype=np.uint32)
    return q_ptr, q_terms


_BASE = {}


def _zipf_base(n_docs=6000, n_terms=40, p_body=60000, p_title=8000, seed=901):
    """Zipf postings, positive tf weights in [1/16, 1], l2 magnitudes: impacts in about [2^-7, 1]."""
    key = (n_docs, n_terms, p_body, p_title, seed)
    if key not in _BASE:
        body = synth.zipf_index(n_docs, n_terms, p_body, seed=seed)
        title = synth.zipf_index(n_docs, n_terms, p_title, seed=seed + 1)
        _BASE[key] = (title, body, _l2(n_docs, title), _l2(n_docs, body))
    return _BASE[key]


def _long_terms(body, at_least=1024):
    t = np.nonzero(np.diff(body[0].astype(np.int64)) >= at_least)[0]
    assert len(t) >= 8
    return t


def _ladder_queries(body, seed):
    """Single-term, 3-term and 3-token-with-a-duplicate queries over the long lists (every kernel takes them)."""
    rng = np.random.default_rng(seed)
    lt = _long_terms(body)
    qs = [[int(t)] for t in rng.choice(lt, size=8, replace=False)]
    qs += [list(map(int, rng.choice(lt, size=3, replace=False))) for _ in range(8)]
    for _ in range(8):
        a, b = map(int, rng.choice(lt, size=2, replace=False))
        qs.append([a, b, a] if rng.random() < 0.5 else [a, a, a])
    return _pack(qs)


# ---- family A: scale ladder ----------------------------------------------------------------------------------------------------
# impacts = base impact (2^-7 .. 1) * 2^t: t = -155 puts all of them below the smallest float32 subnormal 2^-149, -146 / -134 /
# -123 straddle 2^-149 / 2^-137 / 2^-126, 130 straddles FLT_MAX (2^128), 140 puts all of them beyond it.
LADDER = (-155, -146, -134, -123, 0, 100, 130, 140)
A_KS = (1, 5, 64, 128, 513)


def _family_a():
    title, body, mt, mb = _zipf_base()
    n_docs = len(mt)
    q_ptr, q_terms = _ladder_queries(body, 5)
    out = []
    for t in LADDER:                                                             # title and body together
        out.append(EdgeCase(f"A.both{t:+d}", n_docs, title, body, np.ldexp(mt, -t), np.ldexp(mb, -t), q_ptr, q_terms, A_KS))
    for tt, tb in ((130, -146), (-146, 130), (100, -123), (-134, 100), (140, -155)):   # opposite directions
        out.append(EdgeCase(f"A.title{tt:+d}.body{tb:+d}", n_docs, title, body, np.ldexp(mt, -tt), np.ldexp(mb, -tb), q_ptr, q_terms, A_KS))
    rng = np.random.default_rng(17)
    steps = np.array(LADDER)
    per_doc = steps[rng.integers(0, len(steps), size=n_docs)]                      # doc-to-doc differences: every step in one query
    out.append(EdgeCase("A.perdoc", n_docs, title, body, np.ldexp(mt, -per_doc), np.ldexp(mb, -per_doc), q_ptr, q_terms, A_KS, masked=True))
    per_doc_t = steps[rng.integers(0, len(steps), size=n_docs)]
    out.append(EdgeCase("A.perdoc.fields", n_docs, title, body, np.ldexp(mt, -per_doc_t), np.ldexp(mb, -per_doc), q_ptr, q_terms, A_KS))
    # a few docs beyond FLT_MAX among ordinary ones: the winners are exactly the records whose bound saturates
    few = np.zeros(n_docs, dtype=np.int64)
    few[rng.choice(n_docs, size=n_docs // 50, replace=False)] = 140
    few_t = np.zeros(n_docs, dtype=np.int64)
    few_t[rng.choice(n_docs, size=n_docs // 50, replace=False)] = 130
    out.append(EdgeCase("A.fewhuge", n_docs, title, body, np.ldexp(mt, -few_t), np.ldexp(mb, -few), q_ptr, q_terms, A_KS))
    return out


# ---- family B: floor exactness -------------------------------------------------------------------------------------------------

def _family_b():
    """Every list lives on a doc range of its own, so a posting's impact is set freely through its doc's magnitude.
    For k' = 2^j, j = 0 .. 10, lists of k' - 1, k', k' + 1 postings with impacts all equal / all distinct / k' - 1 large and the
    rest tiny; title-only terms; lists padded with weight-0 postings over magnitude 0; one long list of tiny impacts (term
    `filler`: beside it a short list reaches the wave kernel, and the filler is too small to give a floor of its own)."""
    lists_b, w_b, lists_t, w_t = [], [], [], []
    mag_b, mag_t = [], []                                  # per doc, appended range by range
    base = [0]
    queries = []

    def new_range(n, mb, mt=None):
        lo = base[0]
        base[0] += n
        mag_b.append(np.broadcast_to(np.asarray(mb, dtype=np.float64), (n,)).copy())
        mag_t.append(np.zeros(n) if mt is None else np.broadcast_to(np.asarray(mt, dtype=np.float64), (n,)).copy())
        return np.arange(lo, lo + n, dtype=np.uint32)

    def add_term(docs_b, wb, docs_t=None, wt=None):
        lists_b.append(docs_b)
        w_b.append(np.asarray(wb, dtype=np.float32))
        lists_t.append(np.zeros(0, np.uint32) if docs_t is None else docs_t)
        w_t.append(np.zeros(0, np.float32) if wt is None else np.asarray(wt, dtype=np.float32))
        return len(lists_b) - 1

    filler_docs = new_range(2000, 2.0 ** 12)              # impact 2^-12 (k_kth_impact keeps no bound below 2^-8)
    filler = add_term(filler_docs, np.ones(2000))
    short_terms = []
    for j in range(11):
        kp = 1 << j
        for n in (kp - 1, kp, kp + 1):
            i = np.arange(n, dtype=np.float64)
            # equal: the floor's source IS the k-th best score; distinct: impacts in (0.5, 1]; large / tiny: 0.9 and 2^-30
            for mags in (np.full(n, 1.0 + 0.25 * j), 1.0 + i / max(n, 1), np.where(i < kp - 1, 1.0 / 0.9, 2.0 ** 30)):
                short_terms.append(add_term(new_range(n, mags), np.ones(n)))
    for kp in (4, 64, 1024):                               # a term that exists only in the title table
        d = new_range(kp, 1.0, mt=1.0 + np.arange(kp) / kp)
        short_terms.append(add_term(np.zeros(0, np.uint32), np.zeros(0), d, np.ones(kp)))
    zero_terms = []
    for n, n_pos in ((300, 5), (1500, 20)):                # weight 0 over magnitude 0: 0 / 0 = NaN -> 0, rows filled by ascending doc id
        pos = np.zeros(n, dtype=bool)
        pos[np.random.default_rng(n).choice(n, size=n_pos, replace=False)] = True
        d = new_range(n, np.where(pos, 1.0 + np.arange(n) / n, 0.0))
        zero_terms.append(add_term(d, pos.astype(np.float32)))
    for t in short_terms:
        queries.append([t])
        queries.append([t, filler])
    for t in zero_terms:
        queries += [[t], [t, t], [t, short_terms[40]]]
    queries.append([zero_terms[1], filler])
    body = _table(lists_b, w_b)
    title = _table(lists_t, w_t)
    q_ptr, q_terms = _pack(queries)
    return [EdgeCase("B.floor", base[0], title, body, np.concatenate(mag_t), np.concatenate(mag_b), q_ptr, q_terms, K_ALL, masked=True)]


# ---- family C: coefficient spread and clamp --------------------------------------------------------------------------------------

def _family_c():
    """Dense doc range (4096 docs, every list on 40 % of them: sketch slots collide), 66 terms.  Docs 777 and 2048 are in every
    list with weight 1 over magnitude 1 — an impact of 1 where the others stay below 0.4 — so over 12 and more lists their summed
    shares pass the filter's clamp.  Token multiplicity 64 beside 1; 12, 14 .. 24 and 128 lists per query."""
    n_docs, n_terms = 4096, 66
    rng = np.random.default_rng(31)
    champs = np.array([777, 2048])
    lb, wb, lt, wt = [], [], [], []
    for _ in range(n_terms):
        for frac, ll, ww in ((0.40, lb, wb), (0.10, lt, wt)):
            d = np.union1d(np.nonzero(rng.random(n_docs) < frac)[0], champs)
            w = synth.make_tf(len(d), rng)
            w[np.isin(d, champs)] = 1.0
            ll.append(d.astype(np.uint32))
            ww.append(w)
    body, title = _table(lb, wb), _table(lt, wt)
    mb, mt = _l2(n_docs, body), _l2(n_docs, title)
    mb[champs] = 1.0
    mt[champs] = 1.0
    shapes = [[0] * 64 + [1], [2] * 64 + [3, 4], [5, 6] + [5] * 30,
              list(range(6)), list(range(10, 17)), list(range(20, 29)), list(range(30, 42)), list(range(64)),
              list(range(2, 66)), [7], [8, 9, 8]]
    out = []
    q_ptr, q_terms = _pack(shapes)
    ks = (1, 3, 64, 129, 1024)
    out.append(EdgeCase("C.spread", n_docs, title, body, mt, mb, q_ptr, q_terms, ks, masked=True))
    qlens = (1, 2, 3, INT32_MAX, 1_000_000)                  # every shape under every query length
    q_ptr, q_terms = _pack([s for s in shapes for _ in qlens])
    out.append(EdgeCase("C.query_len", n_docs, title, body, mt, mb, q_ptr, q_terms, ks,
                        query_len=np.tile(np.array(qlens, dtype=np.int64), len(shapes))))
    return out


# ---- family D: prior-dominated and prior-negligible blends ------------------------------------------------------------------------
D_KS = (1, 5, 65, 128, 512, 1024)


def _family_d():
    title, body, mt, mb = _zipf_base()
    n_docs, K = len(mt), 4
    rng = np.random.default_rng(43)
    lt = _long_terms(body)
    qs = [list(map(int, rng.choice(lt, size=3, replace=False))) for _ in range(18)] + [[int(t)] for t in rng.choice(lt, size=6, replace=False)]
    q_ptr, q_terms = _pack(qs)
    n_q = len(qs)

    def probs_mixed():
        p = rng.dirichlet(np.ones(K), size=n_q)              # rows that sum to 1 ...
        p[::3] = 0.0                                          # ... and rows that are mostly 0 (one topic)
        p[::3, rng.integers(0, K)] = 1.0
        return p
    out = []
    for scale in (1e-300, 1e-3, 1.0, 1e6, 1e12, 1e300):
        out.append(EdgeCase(f"D.prior{scale:g}", n_docs, title, body, mt, mb, q_ptr, q_terms, D_KS,
                            prior=rng.random((n_docs, K)) * scale, topic_probs=probs_mixed(), masked=(scale == 1e6)))
    # sqd overflows to +Inf: a prior of 1e308 under a row of probabilities that sums to 2 (row 0); the other rows stay finite
    p = probs_mixed() * 1e-3
    p[0] = 0.5
    out.append(EdgeCase("D.sqd_overflow", n_docs, title, body, mt, mb, q_ptr, q_terms, D_KS,
                        prior=np.full((n_docs, K), 1e308) * (0.9 + 0.1 * rng.random((n_docs, K))), topic_probs=p))
    # the term part (at most 67) is absorbed by rounding: 33 * 1e18 has an ulp of 4096, so a tier of equal priors is a tier of
    # EQUAL FinalRanks, broken by ascending doc id; tiers are scattered over the doc range (slice and window boundaries)
    tiers = np.array([1e18, 2e18, 3e18])[rng.integers(0, 3, size=n_docs)]
    onehot = np.zeros((n_q, K))
    onehot[np.arange(n_q), rng.integers(0, K, size=n_q)] = 1.0
    out.append(EdgeCase("D.absorbed_ties", n_docs, title, body, mt, mb, q_ptr, q_terms, D_KS,
                        prior=np.repeat(tiers[:, None], K, axis=1), topic_probs=onehot))
    return out


# ---- family E: phrase part -----------------------------------------------------------------------------------------------------

def _positions(n_post, seed, max_pos):
    """1-3 consecutive positions from a random start per posting, sometimes a -100 anchor entry behind them."""
    rng = np.random.default_rng(seed)
    c = rng.integers(1, 4, size=n_post)
    anchor = rng.random(n_post) < 0.1
    cnt = c + anchor
    pos_ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
    start = rng.integers(0, max_pos, size=n_post).astype(np.float32)
    within = (np.arange(int(pos_ptr[-1])) - np.repeat(pos_ptr[:-1].astype(np.int64), cnt)).astype(np.float32)
    pos = np.repeat(start, cnt) + within
    pos[np.repeat(c, cnt) == within.astype(np.int64)] = np.float32(-100.0)
    return pos_ptr, pos.astype(np.float32)


def _family_e():
    """Phrase records get their impact at run time (k_phrase_match), never seen by the creation-time flags: the ladder's two ends
    and the per-doc mix, with quoted phrases of 2 and 3 terms beside OR terms."""
    n_docs, n_terms = 3000, 12
    body = synth.zipf_index(n_docs, n_terms, 16000, seed=77, q=1000.0, clip_frac=0.9)
    title = synth.zipf_index(n_docs, n_terms, 9000, seed=78, q=1000.0, clip_frac=0.9)
    mt, mb = _l2(n_docs, title), _l2(n_docs, body)
    positions = (_positions(len(title[1]), 5, 3), _positions(len(body[1]), 6, 8))
    cases = [([0, 3], [1, 2]), ([], [0, 1]), ([5], [2, 0]), ([2, 2], [1, 1]), ([4], [0, 99]), ([7, 1], [0, 1, 2]), ([9], []), ([], [3]),
             ([1], [3, 2, 1]), ([6, 8, 10], [4, 5]), ([], [6, 7]), ([11], [8, 9])]
    q_ptr, q_terms = _pack([q for q, _ in cases])
    phrases = _pack([p for _, p in cases])
    rng = np.random.default_rng(3)
    per_doc = np.array(LADDER)[rng.integers(0, len(LADDER), size=n_docs)]
    out = []
    for name, e_t, e_b in (("E.both-155", -155, -155), ("E.both+140", 140, 140), ("E.perdoc", per_doc, per_doc[::-1].copy())):
        out.append(EdgeCase(name, n_docs, title, body, np.ldexp(mt, -np.asarray(e_t)), np.ldexp(mb, -np.asarray(e_b)), q_ptr, q_terms,
                            (1, 5, 64, 129, 513), positions=positions, phrases=phrases, masked=(name == "E.perdoc")))
    return out


_FAMILIES = {"A": _family_a, "B": _family_b, "C": _family_c, "D": _family_d, "E": _family_e}
_CACHE = {}

CASE_NAMES = (
    [f"A.both{t:+d}" for t in LADDER]
    + ["A.title+130.body-146", "A.title-146.body+130", "A.title+100.body-123", "A.title-134.body+100", "A.title+140.body-155",
       "A.perdoc", "A.perdoc.fields", "A.fewhuge"]
    + ["B.floor", "C.spread", "C.query_len"]
    + [f"D.prior{s:g}" for s in (1e-300, 1e-3, 1.0, 1e6, 1e12, 1e300)] + ["D.sqd_overflow", "D.absorbed_ties"]
    + ["E.both-155", "E.both+140", "E.perdoc"])
MASKED_NAMES = ("A.perdoc", "B.floor", "C.spread", "D.prior1e+06", "E.perdoc")     # one masked / constrained call per family


def family(letter):
    """The checked cases of one family (built once per process)."""
    if letter not in _CACHE:
        cases = _FAMILIES[letter]()
        for c in cases:
            c.figures = check_case(c)
            assert c.masked == (c.name in MASKED_NAMES), c.name
        _CACHE[letter] = {c.name: c for c in cases}
    return list(_CACHE[letter].values())


def get_case(name):
    family(name[0])
    return _CACHE[name[0]][name]


def all_cases():
    return [c for letter in _FAMILIES for c in family(letter)]
