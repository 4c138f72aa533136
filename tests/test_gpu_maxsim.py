"""GPU parity: ss_scorer_set_doc_tokens, ss_hit_maxsim_scores and ss_rerank_hits_by_maxsim vs the numpy restatement of the header's
definition (tests/maxsim_model.py).  Scores are exact integers and ties keep the window order, so every comparison is equality of
bytes: tobytes() on whole output arrays that start from 0xA5 bytes, so an entry a call must not write is checked with the ones it must."""
import numpy as np
import pytest

from spaghettisearch_amd import SpaghettiError, engine
from tests import maxsim_model as mm
from tests import vector_model as vm
from tests.test_gpu_collapse import FILL, as_bytes, filled, random_rows
from tests.test_gpu_score import close_all
from tests.test_gpu_vector import tiny_scorer

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE, ERR_UNSUPPORTED = 1, 6, 7
NO = mm.NO_SCORE


def page_outs(n_q, k, scores=True):
    return filled((n_q, k), engine.HIT_DTYPE), filled(n_q, np.int32), filled((n_q, k), np.int32) if scores else None


def rows_of(rng, docs):
    docs = np.asarray(docs)
    hits = random_rows(rng, docs.shape[0], docs.shape[1], 1)      # random bytes in _pad and the scores: carried through
    hits["doc"] = docs
    return hits


def ptr_of(counts, dtype):
    p = np.zeros(len(counts) + 1, dtype)
    p[1:] = np.cumsum(counts)
    return p


class World:
    def __init__(self, ss_ctx, tok_ptr, tok):
        self.tok_ptr, self.tok = tok_ptr, tok
        self.sc, self.ti, self.bi = tiny_scorer(ss_ctx, len(tok_ptr) - 1)
        self.sc.set_doc_tokens(tok_ptr, tok)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        close_all(self.sc, self.ti, self.bi)

    def check(self, qt_ptr, qtok, hits, n_hits, first=0, k=None, tag=None):
        """both calls on host arrays against the model, byte for byte -> (scores, page)"""
        n_q, k_in = hits.shape
        k = k_in if k is None else k
        want = mm.hit_scores(qt_ptr, qtok, self.tok_ptr, self.tok, hits, n_hits, filled((n_q, k_in), np.int32))
        got = self.sc.hit_maxsim_scores(qt_ptr, qtok, hits, n_hits, out=filled((n_q, k_in), np.int32))
        for q in range(n_q):
            assert got[q, :int(n_hits[q])].tolist() == want[q, :int(n_hits[q])].tolist(), (tag, q)
        assert got.tobytes() == want.tobytes(), tag
        want_p = mm.rerank(qt_ptr, qtok, self.tok_ptr, self.tok, hits, n_hits, first, k, *page_outs(n_q, k))
        got_p = self.sc.rerank_hits_by_maxsim(qt_ptr, qtok, hits, n_hits, k, first=first, out=page_outs(n_q, k))
        assert got_p[1].tolist() == want_p[1].tolist(), tag
        assert as_bytes(got_p) == as_bytes(want_p), tag
        return got, got_p


# ---- the known answer ---------------------------------------------------------------------------------------------------------------

def test_known_answer(ss_ctx):
    tok_ptr, tok, qt_ptr, qtok = mm.known_world()
    hits = rows_of(np.random.default_rng(1), [[3, 2, 1, 0, 99]])            # D, C, B, A, doc 99 of a 4-doc table
    n_hits = np.array([5], np.int32)
    with World(ss_ctx, tok_ptr, tok) as w:
        sc, page = w.check(qt_ptr, qtok, hits, n_hits)
        assert sc[0].tolist() == [-11, NO, 12, 16, NO]
        assert page[0]["doc"][0].tolist() == [0, 1, 3, 2, 99] and page[2][0].tolist() == [16, 12, -11, NO, NO]
        assert page[0].tobytes() == hits[:, [3, 2, 0, 1, 4]].tobytes()


# ---- operand layout -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [64, 192])
def test_operand_layout(ss_ctx, dim):
    """one-hot doc tokens against dense query tokens with a distinct value per position, and the reverse: a dot product is one product,
    so a permuted k order on one operand, a row / column swap or an unsummed k step each give wrong maxima"""
    rng = np.random.default_rng(dim)
    i = np.arange(dim)
    dense = np.stack([((i * 37 + x * 11) % 251) - 125 for x in range(12)]).astype(np.int8)
    assert all(len(set(r.tolist())) == 64 for r in dense[:, :64])
    n_hot_docs, per_doc = dim, 3
    hot = np.zeros((n_hot_docs * per_doc, dim), np.int8)
    t = np.arange(len(hot))
    hot[t, (t * 5 + t // dim) % dim] = 1 + t % 7                            # every position is hot in some token
    assert (hot != 0).any(axis=0).all()
    n_dense_docs = 4
    tok = np.concatenate([hot, dense[:2 * n_dense_docs]])
    tok_ptr = ptr_of([per_doc] * n_hot_docs + [2] * n_dense_docs, np.uint64)
    n_docs = n_hot_docs + n_dense_docs
    # query 0: dense tokens; query 1: one-hot tokens, one per position 0, 3, 6, ..; query 2: both kinds
    q_hot = np.zeros((20, dim), np.int8)
    q_hot[np.arange(20), (np.arange(20) * 3) % dim] = np.arange(20) % 5 + 1
    qtok = np.concatenate([dense[8:12], q_hot, dense[9:11], q_hot[:3]])
    qt_ptr = ptr_of([4, 20, 5], np.uint32)
    docs = np.stack([rng.permutation(n_docs) for _ in range(3)])
    hits = rows_of(rng, docs)
    n_hits = np.full(3, n_docs, np.int32)
    with World(ss_ctx, tok_ptr, tok) as w:
        sc, _ = w.check(qt_ptr, qtok, hits, n_hits, tag=dim)
        assert len(np.unique(sc[0])) > 20                                   # the scores are many different sums


# ---- token-count seams --------------------------------------------------------------------------------------------------------------

T_SEAMS = [0, 1, 15, 16, 17, 63, 64, 65, 130]


@pytest.mark.parametrize("m_q", [3, 20, 40])
def test_token_count_seams(ss_ctx, m_q):
    """every true dot product is negative, so a padded slot that leaks a 0 changes the score; the maximum (the one token of small
    values) sits at the first token, at the last token — for T no multiple of 16 the last token of a partial tile — or in between"""
    dim = 64
    rng = np.random.default_rng(m_q)
    rows, counts = [], []
    for T in T_SEAMS:
        for where in ("first", "last", "any"):
            block = rng.integers(60, 128, (T, dim)).astype(np.int8)
            if T:
                block[{"first": 0, "last": T - 1, "any": int(rng.integers(0, T))}[where]] = rng.integers(1, 4, dim)
            rows.append(block)
            counts.append(T)
    tok, tok_ptr = np.concatenate(rows), ptr_of(counts, np.uint64)
    n_docs = len(counts)
    qtok = -rng.integers(1, 128, (m_q + 2, dim)).astype(np.int8)
    qt_ptr = np.array([0, m_q, m_q + 2], np.uint32)
    hits = rows_of(rng, np.stack([np.arange(n_docs), rng.permutation(n_docs)]))
    n_hits = np.full(2, n_docs, np.int32)
    with World(ss_ctx, tok_ptr, tok) as w:
        sc, _ = w.check(qt_ptr, qtok, hits, n_hits, tag=m_q)
        assert ((sc < 0)).all() and (sc[0, :3] == NO).all() and (sc[0, 3:] != NO).all()
        # the small token decides: a doc's score is the same wherever that token sits, given the same token
        small = -qtok[:m_q].astype(np.int64)
        for d in range(3, n_docs):
            lo = int(tok_ptr[d])
            best = tok[lo:int(tok_ptr[d + 1])].astype(np.int64).sum(axis=1).argmin()
            assert sc[0, d] == -int((small @ tok[lo + best].astype(np.int64)).sum())


# ---- query-token seams --------------------------------------------------------------------------------------------------------------

M_SEAMS = [0, 1, 15, 16, 17, 32, 33, 64]


def query_seam_world(rng, dim=64, n_docs=40):
    counts = rng.integers(0, 40, n_docs)
    counts[:4] = [0, 1, 16, 17]
    tok = rng.integers(1, 128, (int(counts.sum()), dim)).astype(np.int8)      # positive: a slot past m_q that is summed adds to the score
    return ptr_of(counts, np.uint64), tok


@pytest.mark.parametrize("m_q", M_SEAMS)
def test_query_token_seams_one_value_per_call(ss_ctx, m_q):
    rng = np.random.default_rng(100 + m_q)
    tok_ptr, tok = query_seam_world(rng)
    n_docs = len(tok_ptr) - 1
    qtok = rng.integers(1, 128, (2 * m_q + 5, 64)).astype(np.int8)            # rows behind the last query's: never read
    qt_ptr = np.array([0, m_q, 2 * m_q], np.uint32)
    hits = rows_of(rng, np.stack([rng.permutation(n_docs), rng.permutation(n_docs)]))
    with World(ss_ctx, tok_ptr, tok) as w:
        sc, _ = w.check(qt_ptr, qtok, hits, np.array([n_docs, 7], np.int32), tag=m_q)
        if m_q == 0:
            assert set(sc[0].tolist()) == {0, NO}


def test_query_token_seams_mixed_in_one_call(ss_ctx):
    """queries below the call's QT: the slots past m_q hold nothing of the next query's tokens"""
    rng = np.random.default_rng(99)
    tok_ptr, tok = query_seam_world(rng)
    n_docs = len(tok_ptr) - 1
    for order in (M_SEAMS, M_SEAMS[::-1], [1, 64, 0, 33, 15, 32, 17, 16], [0, 1, 15, 16], [17, 0, 32, 1]):
        qt_ptr = ptr_of(order, np.uint32) + np.uint32(3)                        # (qt_ptr need not start at 0)
        qtok = rng.integers(1, 128, (int(qt_ptr[-1]) + 4, 64)).astype(np.int8)
        hits = rows_of(rng, np.stack([rng.permutation(n_docs) for _ in order]))
        n_hits = rng.integers(1, n_docs + 1, len(order)).astype(np.int32)
        with World(ss_ctx, tok_ptr, tok) as w:
            w.check(qt_ptr, qtok, hits, n_hits, tag=order)


# ---- extremes -----------------------------------------------------------------------------------------------------------------------

def test_extremes(ss_ctx):
    dim = 1024
    tok_ptr = np.array([0, 1, 4, 4, 70], np.uint64)
    tok = np.full((70, dim), -128, np.int8)
    tok[3] = 127                                                            # doc 1: two tokens of -128 and one of 127
    qtok = np.concatenate([np.full((64, dim), -128, np.int8), np.full((64, dim), 127, np.int8)])
    qt_ptr = np.array([0, 64, 128], np.uint32)
    hits = rows_of(np.random.default_rng(5), [[0, 1, 2, 3], [3, 2, 1, 0]])
    with World(ss_ctx, tok_ptr, tok) as w:
        sc, _ = w.check(qt_ptr, qtok, hits, np.array([4, 4], np.int32))
        assert sc[0].tolist() == [2 ** 30, 2 ** 30, NO, 2 ** 30]
        assert sc[1].tolist() == [-64 * 1024 * 127 * 128, NO, 64 * 1024 * 127 * 127, -64 * 1024 * 127 * 128]


# ---- wide rows ----------------------------------------------------------------------------------------------------------------------

def test_wide_rows_give_the_same_bytes(ss_ctx):
    rng = np.random.default_rng(41)
    dim = 64
    counts = [1, 64, 257, 1000, 0, 63, 65, 256, 1, 257]
    tok_ptr = ptr_of(counts, np.uint64)
    tok = rng.integers(-128, 128, (int(tok_ptr[-1]), dim)).astype(np.int8)
    tok[int(tok_ptr[3]):int(tok_ptr[4])] = -rng.integers(1, 128, (1000, dim))    # doc 3 against query 2: every dot product negative
    n_docs = len(counts)
    qt_ptr = ptr_of([20, 3, 40], np.uint32)
    qtok = rng.integers(-128, 128, (63, dim)).astype(np.int8)
    qtok[23:] = rng.integers(1, 128, (40, dim))
    docs = np.stack([rng.integers(0, n_docs + 1, 70) for _ in range(3)])       # 70 rows: two workgroups a query; one row outside the table
    docs[:, :4] = [0, 1, 2, 3]
    hits = rows_of(rng, docs)
    n_hits = np.array([70, 70, 66], np.int32)
    with World(ss_ctx, tok_ptr, tok) as w:
        try:
            base = None
            for wide in (1, None, 2 ** 30, 257, 64, 2 ** 40):
                ss_ctx.set_option("maxsim.wide_tokens", wide)
                sc, page = w.check(qt_ptr, qtok, hits, n_hits, tag=wide)
                got = as_bytes((sc,) + tuple(page))
                base = base or got
                assert got == base, wide
        finally:
            ss_ctx.set_option("maxsim.wide_tokens", None)


# ---- window edges -------------------------------------------------------------------------------------------------------------------

def edge_world(seed=29, n_docs=300, dim=64):
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 9, n_docs)
    tok_ptr = ptr_of(counts, np.uint64)
    tok = rng.integers(-2, 3, (int(tok_ptr[-1]), dim)).astype(np.int8)
    tok[:, 3:] = 0                                                           # few distinct scores: equal scores inside every window
    return tok_ptr, tok, rng


def test_window_edges(ss_ctx):
    tok_ptr, tok, rng = edge_world()
    n_docs, k_in = len(tok_ptr) - 1, 140
    qt_ptr = ptr_of([2, 0, 5, 17], np.uint32)
    qtok = rng.integers(-2, 3, (24, 64)).astype(np.int8)
    docs = rng.integers(0, n_docs, (4, k_in))
    docs[:, 3] = docs[:, 77]                                                # the same doc twice
    docs[:, 4] = docs[:, 5]
    docs[0, [0, 9, 64, 100, 139]] = [n_docs, 0xFFFFFFFF, n_docs + 1, 0x80000000, n_docs]
    docs[2, :] = rng.integers(n_docs, 2 ** 32, k_in)                        # an all-outside window
    hits = rows_of(rng, docs)
    with World(ss_ctx, tok_ptr, tok) as w:
        for n_hits in (np.array([k_in, k_in, k_in, 67], np.int32), np.array([0, 1, 0, k_in], np.int32)):
            for first in (0, 3, 66, 67, 139, 140, 141, 5000):
                for k in (1, 7, 1024):
                    w.check(qt_ptr, qtok, hits, n_hits, first=first, k=k, tag=(first, k))
        sc, page = w.check(qt_ptr, qtok, hits, np.full(4, k_in, np.int32))
        q = 0                                                               # equal scores stay in window order; rows without a score last
        order = sorted(range(k_in), key=lambda j: (sc[q, j] == NO, -int(sc[q, j]), j))
        assert page[0][q].tobytes() == hits[q, order].tobytes() and len(set(sc[q].tolist())) < k_in // 2
        assert page[0][2].tobytes() == hits[2].tobytes() and set(page[2][2].tolist()) == {NO}
        # scores_out is optional
        got = w.sc.rerank_hits_by_maxsim(qt_ptr, qtok, hits, np.full(4, k_in, np.int32), 10, first=2, out=page_outs(4, 10, scores=False))
        want = mm.rerank(qt_ptr, qtok, tok_ptr, tok, hits, np.full(4, k_in, np.int32), 2, 10, *page_outs(4, 10, scores=False))
        assert as_bytes(got) == as_bytes(want)


@pytest.mark.parametrize("k_in", [1, 1024])
def test_window_widths(ss_ctx, k_in):
    tok_ptr, tok, rng = edge_world(seed=k_in)
    n_docs = len(tok_ptr) - 1
    qt_ptr = ptr_of([4, 1, 33], np.uint32)
    qtok = rng.integers(-2, 3, (38, 64)).astype(np.int8)
    hits = rows_of(rng, rng.integers(0, n_docs + 5, (3, k_in)))
    with World(ss_ctx, tok_ptr, tok) as w:
        for n_hits in ([k_in, k_in, k_in], [0, k_in, k_in // 2]):
            w.check(qt_ptr, qtok, hits, np.array(n_hits, np.int32), tag=(k_in, n_hits))
        w.check(qt_ptr, qtok, hits, np.full(3, k_in, np.int32), first=k_in // 2, k=10)


# ---- one token per doc and per query: the doc-vector calls ----------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [64, 192])
def test_one_token_tables_are_the_vector_calls(ss_ctx, dim):
    rng = np.random.default_rng(dim + 1)
    n_docs, n_q, k_in = 200, 5, 70
    vec = rng.integers(-128, 128, (n_docs, dim)).astype(np.int8)
    vec[:50, 2:] = 0                                                        # equal scores among the first docs
    qvec = rng.integers(-128, 128, (n_q, dim)).astype(np.int8)
    hits = rows_of(rng, rng.integers(0, n_docs + 3, (n_q, k_in)))
    hits["doc"][:, :30] = rng.integers(0, 50, (n_q, 30))
    n_hits = np.array([k_in, k_in - 7, 0, 1, k_in], np.int32)
    tok_ptr, qt_ptr = np.arange(n_docs + 1, dtype=np.uint64), np.arange(n_q + 1, dtype=np.uint32)
    with World(ss_ctx, tok_ptr, vec) as w:
        w.sc.set_doc_vectors(vec)
        a = w.sc.hit_maxsim_scores(qt_ptr, qvec, hits, n_hits, out=filled((n_q, k_in), np.int32))
        b = w.sc.hit_vector_scores(qvec, hits, n_hits, out=filled((n_q, k_in), np.int32))
        assert a.tobytes() == b.tobytes() == vm.hit_scores(qvec, vec, hits, n_hits, filled((n_q, k_in), np.int32)).tobytes()
        for first, k in ((0, k_in), (5, 10), (60, 20)):
            a = w.sc.rerank_hits_by_maxsim(qt_ptr, qvec, hits, n_hits, k, first=first, out=page_outs(n_q, k))
            b = w.sc.rerank_hits_by_vector(qvec, hits, n_hits, k, first=first, out=page_outs(n_q, k))
            assert as_bytes(a) == as_bytes(b)


# ---- memory kinds -------------------------------------------------------------------------------------------------------------------

def test_memory_kinds(ss_ctx):
    import torch
    tok_ptr, tok, rng = edge_world(seed=31)
    n_docs, n_q, k_in = len(tok_ptr) - 1, 4, 140
    qt_ptr = ptr_of([2, 0, 5, 17], np.uint32)
    qtok = rng.integers(-2, 3, (24, 64)).astype(np.int8)
    hits = rows_of(rng, rng.integers(0, n_docs + 9, (n_q, k_in)))
    dev = lambda a: torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).cuda()      # noqa: E731
    sc, ti, bi = tiny_scorer(ss_ctx, n_docs)
    try:
        sc.set_doc_tokens(torch.from_numpy(tok_ptr.view(np.int64)).cuda(), torch.from_numpy(tok).cuda())     # a table from device memory
        d_hits, d_q = dev(hits), torch.from_numpy(qtok).cuda()
        odd = torch.zeros(qtok.size + 1, dtype=torch.int8, device="cuda")
        odd[1:] = torch.from_numpy(qtok.reshape(-1)).cuda()
        d_q_odd = odd[1:].view(len(qtok), -1)                    # query tokens at an odd address
        assert d_q_odd.data_ptr() % 16 == 1
        for counts in (np.array([k_in, 3, k_in, 67], np.int32), np.array([-5, k_in + 9, 2, k_in], np.int32)):   # device counts are clamped
            for first, k in ((0, k_in), (4, 9)):
                want_s = mm.hit_scores(qt_ptr, qtok, tok_ptr, tok, hits, counts, filled((n_q, k_in), np.int32), clamp=True)
                want_p = mm.rerank(qt_ptr, qtok, tok_ptr, tok, hits, counts, first, k, *page_outs(n_q, k), clamp=True)
                d_n = dev(counts)
                for dq in (d_q, d_q_odd):
                    # all device: the calls only enqueue; the page's rows are scored again behind it on the same stream
                    d_s, d_p, d_s2 = dev(filled((n_q, k_in), np.int32)), tuple(dev(a) for a in page_outs(n_q, k)), dev(filled((n_q, k), np.int32))
                    sc.hit_maxsim_scores(qt_ptr, dq, d_hits, d_n, k_in=k_in, out=d_s)
                    sc.rerank_hits_by_maxsim(qt_ptr, dq, d_hits, d_n, k, first=first, k_in=k_in, out=d_p)
                    sc.hit_maxsim_scores(qt_ptr, dq, d_p[0], d_p[1], k_in=k, out=d_s2)
                    assert d_s.cpu().numpy().tobytes() == want_s.tobytes()
                    assert [t.cpu().numpy().tobytes() for t in d_p] == as_bytes(want_p), (first, k)
                    assert d_s2.cpu().numpy().tobytes() == want_p[2].tobytes()
                got = sc.hit_maxsim_scores(qt_ptr, qtok, hits, d_n, k_in=k_in, out=filled((n_q, k_in), np.int32))   # host rows, device counts
                assert got.tobytes() == want_s.tobytes()
                h_out = page_outs(n_q, k)
                mixed = (dev(h_out[0]), h_out[1], dev(h_out[2]))
                sc.rerank_hits_by_maxsim(qt_ptr, d_q, hits, d_n, k, first=first, k_in=k_in, out=mixed)              # device rows out, host counts out
                assert [mixed[0].cpu().numpy().tobytes(), mixed[1].tobytes(), mixed[2].cpu().numpy().tobytes()] == as_bytes(want_p)
        # host counts outside the window are refused, outputs untouched
        for bad in (np.array([-5, 1, 1, 1], np.int32), np.array([1, k_in + 9, 1, 1], np.int32)):
            o, o_s = page_outs(n_q, 5), filled((n_q, k_in), np.int32)
            with pytest.raises(SpaghettiError) as ei:
                sc.rerank_hits_by_maxsim(qt_ptr, qtok, hits, bad, 5, out=o)
            assert ei.value.code == ERR_INVALID and as_bytes(o) == as_bytes(page_outs(n_q, 5))
            with pytest.raises(SpaghettiError) as ei:
                sc.hit_maxsim_scores(qt_ptr, qtok, hits, bad, out=o_s)
            assert ei.value.code == ERR_INVALID and o_s.tobytes() == bytes([FILL]) * o_s.nbytes
    finally:
        close_all(sc, ti, bi)


# ---- lifecycle and refusals ---------------------------------------------------------------------------------------------------------

def test_lifecycle(ss_ctx):
    tok_ptr, tok, rng = edge_world(seed=37, n_docs=120)
    n_docs, n_q, k_in = len(tok_ptr) - 1, 3, 30
    qt_ptr = ptr_of([2, 5, 17], np.uint32)
    qtok = rng.integers(-2, 3, (24, 64)).astype(np.int8)
    hits = rows_of(rng, rng.integers(0, n_docs, (n_q, k_in)))
    n_hits = np.full(n_q, k_in, np.int32)
    score = lambda sc: sc.hit_maxsim_scores(qt_ptr, qtok, hits, n_hits, out=filled((n_q, k_in), np.int32))      # noqa: E731
    model = lambda tp, t: mm.hit_scores(qt_ptr, qtok, tp, t, hits, n_hits, filled((n_q, k_in), np.int32))       # noqa: E731
    sc, ti, bi = tiny_scorer(ss_ctx, n_docs)
    try:
        with pytest.raises(SpaghettiError) as ei:
            score(sc)
        assert ei.value.code == ERR_STATE                                   # before a table exists
        sc.set_doc_tokens(tok_ptr, tok)
        first = score(sc)
        assert first.tobytes() == model(tok_ptr, tok).tobytes()
        # the doc vectors are another table: registering or clearing them leaves the tokens alone, and the reverse
        vec = rng.integers(-128, 128, (n_docs, 128)).astype(np.int8)
        qvec = rng.integers(-128, 128, (n_q, 128)).astype(np.int8)
        sc.set_doc_vectors(vec)
        by_vec = sc.hit_vector_scores(qvec, hits, n_hits, out=filled((n_q, k_in), np.int32))
        assert score(sc).tobytes() == first.tobytes()
        sc.set_doc_vectors(None)
        assert score(sc).tobytes() == first.tobytes()
        sc.set_doc_vectors(vec)
        # a new table replaces the old one: the scores change
        tok_ptr2 = ptr_of(rng.integers(0, 5, n_docs), np.uint64)
        tok2 = rng.integers(-9, 10, (int(tok_ptr2[-1]), 128)).astype(np.int8)
        sc.set_doc_tokens(tok_ptr2, tok2)
        with pytest.raises(ValueError):
            score(sc)                                                       # (the engine knows the new dim: 64-wide query tokens are refused)
        qtok2 = rng.integers(-9, 10, (24, 128)).astype(np.int8)
        second = sc.hit_maxsim_scores(qt_ptr, qtok2, hits, n_hits, out=filled((n_q, k_in), np.int32))
        assert second.tobytes() == mm.hit_scores(qt_ptr, qtok2, tok_ptr2, tok2, hits, n_hits, filled((n_q, k_in), np.int32)).tobytes()
        assert second.tobytes() != first.tobytes()
        assert sc.hit_vector_scores(qvec, hits, n_hits, out=filled((n_q, k_in), np.int32)).tobytes() == by_vec.tobytes()
        # a failing call leaves the old table in place
        bad_ptr = tok_ptr2.copy()
        bad_ptr[0] = 1
        with pytest.raises(SpaghettiError) as ei:
            sc.set_doc_tokens(bad_ptr, tok2)
        assert ei.value.code == ERR_INVALID
        assert sc.hit_maxsim_scores(qt_ptr, qtok2, hits, n_hits, out=filled((n_q, k_in), np.int32)).tobytes() == second.tobytes()
        sc.set_doc_tokens(None, None)
        with pytest.raises(SpaghettiError) as ei:
            sc.hit_maxsim_scores(qt_ptr, qtok2, hits, n_hits)
        assert ei.value.code == ERR_STATE                                   # after it is cleared
        assert sc.hit_vector_scores(qvec, hits, n_hits, out=filled((n_q, k_in), np.int32)).tobytes() == by_vec.tobytes()
    finally:
        close_all(sc, ti, bi)


def test_errors_leave_outputs_untouched(ss_ctx):
    n_docs, dim, n_q, k = 50, 64, 4, 5
    rng = np.random.default_rng(23)
    tok_ptr = ptr_of(rng.integers(0, 4, n_docs), np.uint64)
    tok = rng.integers(-128, 128, (int(tok_ptr[-1]), dim)).astype(np.int8)
    qt_ptr = ptr_of([1, 0, 3, 2], np.uint32)
    qtok = rng.integers(-128, 128, (70, dim)).astype(np.int8)
    hits = random_rows(rng, n_q, k, n_docs)
    n_hits = np.full(n_q, k, np.int32)
    lib = ss_ctx.lib
    ptr = lambda a: None if a is None else a.ctypes.data        # noqa: E731
    sc, ti, bi = tiny_scorer(ss_ctx, n_docs)
    try:
        o_h, o_n, o_s = page_outs(n_q, k)
        o_e = filled((n_q, k), np.int32)
        clean = as_bytes((o_h, o_n, o_s, o_e))
        rerank = lambda nq=n_q, qp=qt_ptr, q=qtok, ki=k, h=hits, n=n_hits, first=0, kk=k, oh=o_h, on=o_n, os_=o_s: lib.ss_rerank_hits_by_maxsim(   # noqa: E731
            sc.h, nq, ptr(qp), ptr(q), ki, ptr(h), ptr(n), first, kk, ptr(oh), ptr(on), ptr(os_))
        scores = lambda nq=n_q, qp=qt_ptr, q=qtok, ki=k, h=hits, n=n_hits, o=o_e: lib.ss_hit_maxsim_scores(   # noqa: E731
            sc.h, nq, ptr(qp), ptr(q), ki, ptr(h), ptr(n), ptr(o))
        assert rerank() == ERR_STATE and scores() == ERR_STATE                          # no token table
        assert rerank(kk=0) == ERR_INVALID and scores(ki=0) == ERR_INVALID              # (the arguments are checked before the state)
        assert as_bytes((o_h, o_n, o_s, o_e)) == clean
        # the table's own refusals: none of them registers anything
        set_tokens = lambda d=dim, tp=tok_ptr, t=tok: lib.ss_scorer_set_doc_tokens(sc.h, d, ptr(tp), ptr(t))      # noqa: E731
        dec = tok_ptr.copy()
        dec[7] = dec[6] - 1 if dec[6] else dec[8] + 1
        one = tok_ptr.copy()
        one[0] = 1
        huge = tok_ptr.copy()
        huge[n_docs] = huge[n_docs - 1] + 2 ** 31                                       # a doc of 2^31 tokens: refused before tok is read
        for rc, bad in ((ERR_INVALID, lambda: set_tokens(d=96)), (ERR_INVALID, lambda: set_tokens(d=1088)), (ERR_INVALID, lambda: set_tokens(d=-64)),
                        (ERR_INVALID, lambda: set_tokens(d=32)), (ERR_INVALID, lambda: set_tokens(tp=one)), (ERR_INVALID, lambda: set_tokens(tp=dec)),
                        (ERR_INVALID, lambda: set_tokens(tp=None)), (ERR_UNSUPPORTED, lambda: set_tokens(tp=huge)),
                        (ERR_INVALID, lambda: lib.ss_scorer_set_doc_tokens(None, dim, ptr(tok_ptr), ptr(tok)))):
            assert bad() == rc
            assert scores() == ERR_STATE
        assert set_tokens() == 0
        up = qt_ptr.copy()
        up[2] = up[1] + 65                                                              # 65 query tokens
        up[3:] = up[2]
        down = qt_ptr.copy()
        down[2] = 0                                                                     # a decreasing pointer
        for rc, bad in ((ERR_INVALID, lambda: lib.ss_rerank_hits_by_maxsim(None, n_q, ptr(qt_ptr), ptr(qtok), k, ptr(hits), ptr(n_hits), 0, k, ptr(o_h),
                                                                           ptr(o_n), ptr(o_s))),
                        (ERR_INVALID, lambda: lib.ss_hit_maxsim_scores(None, n_q, ptr(qt_ptr), ptr(qtok), k, ptr(hits), ptr(n_hits), ptr(o_e))),
                        (ERR_INVALID, lambda: rerank(nq=-1)), (ERR_INVALID, lambda: rerank(ki=0)), (ERR_INVALID, lambda: rerank(kk=0)),
                        (ERR_INVALID, lambda: rerank(first=-1)), (ERR_UNSUPPORTED, lambda: rerank(ki=1025)), (ERR_UNSUPPORTED, lambda: rerank(kk=1025)),
                        (ERR_INVALID, lambda: rerank(h=None)), (ERR_INVALID, lambda: rerank(n=None)), (ERR_INVALID, lambda: rerank(oh=None)),
                        (ERR_INVALID, lambda: rerank(on=None)), (ERR_INVALID, lambda: rerank(qp=None)), (ERR_INVALID, lambda: rerank(q=None)),
                        (ERR_INVALID, lambda: rerank(qp=down)), (ERR_UNSUPPORTED, lambda: rerank(qp=up)),
                        (ERR_INVALID, lambda: rerank(n=np.array([k + 1, 0, 0, 0], np.int32))), (ERR_INVALID, lambda: rerank(n=np.array([0, 0, -1, 0], np.int32))),
                        (ERR_INVALID, lambda: scores(nq=-1)), (ERR_INVALID, lambda: scores(ki=0)), (ERR_UNSUPPORTED, lambda: scores(ki=1025)),
                        (ERR_INVALID, lambda: scores(h=None)), (ERR_INVALID, lambda: scores(n=None)), (ERR_INVALID, lambda: scores(o=None)),
                        (ERR_INVALID, lambda: scores(qp=None)), (ERR_INVALID, lambda: scores(q=None)), (ERR_INVALID, lambda: scores(qp=down)),
                        (ERR_UNSUPPORTED, lambda: scores(qp=up)), (ERR_INVALID, lambda: scores(n=np.array([k + 1, 0, 0, 0], np.int32)))):
            assert bad() == rc
            assert as_bytes((o_h, o_n, o_s, o_e)) == clean
        both = filled((n_q, 2 * k), engine.HIT_DTYPE)
        assert lib.ss_rerank_hits_by_maxsim(sc.h, n_q, ptr(qt_ptr), ptr(qtok), k, ptr(both), ptr(n_hits), 0, k, both.ctypes.data + 40, ptr(o_n),
                                            None) == ERR_INVALID                        # hits_out overlaps hits
        assert as_bytes((o_h, o_n, o_s, o_e)) == clean and both.tobytes() == bytes([FILL]) * both.nbytes
        assert rerank(nq=0) == 0 and scores(nq=0) == 0 and rerank(nq=0, qp=None, q=None) == 0 and as_bytes((o_h, o_n, o_s, o_e)) == clean
        assert rerank(os_=None) == 0 and o_s.tobytes() == clean[2]                      # scores_out is optional
        none = np.zeros(n_q + 1, np.uint32)
        assert scores(qp=none, q=None) == 0                                             # no query has a token: qtok may be NULL
        assert o_e.tolist() == mm.hit_scores(none, qtok, tok_ptr, tok, hits, n_hits, filled((n_q, k), np.int32)).tolist()
        assert rerank() == 0 and scores() == 0
        with pytest.raises(SpaghettiError):
            ss_ctx.set_option("maxsim.no_such_option", 1)
    finally:
        close_all(sc, ti, bi)
