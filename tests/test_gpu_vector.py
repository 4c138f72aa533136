"""GPU parity: doc vectors (ss_scorer_set_doc_vectors, ss_vector_topk, ss_hit_vector_scores, ss_rerank_hits_by_vector) vs the numpy
restatement of the header's definitions (tests/vector_model.py).  Scores are exact 32-bit integers and ties break by doc id, so every
comparison is equality of bytes: tobytes() on whole output arrays that start from 0xA5 bytes, so an entry a call must not write is
checked with the ones it must."""
import numpy as np
import pytest

from spaghettisearch_amd import SpaghettiError, engine
from tests import vector_model as vm
from tests.test_gpu_collapse import FILL, as_bytes, filled, random_rows
from tests.test_gpu_score import close_all, make_scorer

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE, ERR_UNSUPPORTED = 1, 6, 7
TILE = 64                        # docs of one wave step of k_vec_topk: ss::vec::TILE (test_vector_cpu.py reads it in vector_plan.hpp)
TINY = (np.array([0, 1], np.uint64), np.array([0], np.uint32), np.array([1.0], np.float32))      # one posting: the tables do not matter


def tiny_scorer(ss_ctx, n_docs):
    return make_scorer(ss_ctx, n_docs, TINY, TINY, np.ones(n_docs), np.ones(n_docs))


def window_of_all(n_q, n_docs):
    """windows that list every doc, SS_MAX_TOPK rows at a time -> list of (hits, n_hits)"""
    out = []
    for lo in range(0, n_docs, 1024):
        n = min(1024, n_docs - lo)
        hits = np.zeros((n_q, n), engine.HIT_DTYPE)
        hits["doc"][:] = np.arange(lo, lo + n)
        out.append((hits, np.full(n_q, n, np.int32)))
    return out


def check_topk(sc, qvec, vec, k, mask_id=None, masks=None, tag=None):
    n_q = qvec.shape[0]
    want = vm.topk(qvec, vec, k, filled((n_q, k), engine.VEC_HIT_DTYPE), filled(n_q, np.int32), mask_id, masks)
    got = sc.vector_topk(qvec, k, mask_id, out=(filled((n_q, k), engine.VEC_HIT_DTYPE), filled(n_q, np.int32)))
    assert got[1].tolist() == want[1].tolist(), tag
    for q in range(n_q):
        n = int(want[1][q])
        assert got[0][q, :n].tolist() == want[0][q, :n].tolist(), (tag, q)
    assert as_bytes(got) == as_bytes(want), tag
    return got


def check_all_scores(sc, qvec, vec):
    sc_all = vm.scores(qvec, vec)
    for hits, n_hits in window_of_all(qvec.shape[0], vec.shape[0]):
        got = sc.hit_vector_scores(qvec, hits, n_hits, out=filled(hits.shape, np.int32))
        lo = int(hits["doc"][0, 0])
        assert got.tobytes() == sc_all[:, lo:lo + hits.shape[1]].astype(np.int32).tobytes()


# ---- operand layout -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [64, 192])
def test_operand_layout(ss_ctx, dim):
    """one-hot docs against queries with a distinct weight per position: a permuted k order, a row / column swap or an unsummed k step
    each give wrong scores"""
    n_docs, n_q = 3 * dim + 5, 17
    vec = np.zeros((n_docs, dim), np.int8)
    d = np.arange(n_docs)
    vec[d, d % dim] = 1 + d % 7
    i = np.arange(dim)
    qvec = np.stack([((i * 37 + q * 11) % 251) - 125 for q in range(n_q)]).astype(np.int8)
    assert len({tuple(r) for r in qvec}) == n_q and all(len(set(r.tolist())) == 64 for r in qvec[:, :64])
    sc, ti, bi = tiny_scorer(ss_ctx, n_docs)
    try:
        sc.set_doc_vectors(vec)
        check_all_scores(sc, qvec, vec)
        for k in (1, 10, n_docs):
            check_topk(sc, qvec, vec, k, tag=(dim, k))
    finally:
        close_all(sc, ti, bi)


# ---- shapes -------------------------------------------------------------------------------------------------------------------------

SHAPES = [(1, 64, 1, 1), (63, 128, 17, 10), (64, 64, 33, 1024), (65, 192, 1, 10), (1000, 128, 33, 10), (1000, 1024, 17, 1),
          (4099, 64, 17, 1024), (4099, 192, 33, 10), (4099, 1024, 33, 1024), (63, 1024, 1, 1024), (65, 64, 33, 1)]


@pytest.mark.parametrize("n_docs,dim,n_q,k", SHAPES)
def test_shapes(ss_ctx, n_docs, dim, n_q, k):
    rng = np.random.default_rng(n_docs * 7 + dim + n_q + k)
    vec = rng.integers(-128, 128, (n_docs, dim)).astype(np.int8)
    qvec = rng.integers(-128, 128, (n_q, dim)).astype(np.int8)
    sc, ti, bi = tiny_scorer(ss_ctx, n_docs)
    try:
        sc.set_doc_vectors(vec)
        check_topk(sc, qvec, vec, k, tag=(n_docs, dim, n_q, k))
        check_all_scores(sc, qvec[:3], vec)
    finally:
        close_all(sc, ti, bi)


def test_shape_grid_holds_every_value():
    cols = list(zip(*SHAPES))
    assert set(cols[0]) == {1, 63, 64, 65, 1000, 4099} and set(cols[1]) == {64, 128, 192, 1024}
    assert set(cols[2]) == {1, 17, 33} and set(cols[3]) == {1, 10, 1024}
    assert (1, 64, 1, 1) in SHAPES and (4099, 1024, 33, 1024) in SHAPES


# ---- value edges --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [64, 1024])
def test_value_edges(ss_ctx, dim):
    n_docs = 130
    vec = np.full((n_docs, dim), -128, np.int8)
    half = np.where(np.arange(dim) % 2 == 0, 127, -127).astype(np.int8)
    vec[100:] = half                                           # mixed signs: against an all-127 query the exact sum is 0
    qvec = np.stack([np.full(dim, -128, np.int8), np.full(dim, 127, np.int8), half])
    want = vm.scores(qvec, vec)
    assert want[0, 0] == dim * 16384 and want[1, 0] == -128 * 127 * dim and want[1, 100] == 0 and want[2, 100] == 127 * 127 * dim
    if dim == 1024:
        assert want[0, 0] == 2 ** 24
    sc, ti, bi = tiny_scorer(ss_ctx, n_docs)
    try:
        sc.set_doc_vectors(vec)
        check_all_scores(sc, qvec, vec)
        for k in (1, 100, 101, 130):
            check_topk(sc, qvec, vec, k, tag=(dim, k))
    finally:
        close_all(sc, ti, bi)


# ---- ties ---------------------------------------------------------------------------------------------------------------------------

def ties_world(seed=5, n_docs=4099, dim=64, n_q=17, seam=256):
    rng = np.random.default_rng(seed)
    vec = rng.integers(-1, 2, (n_docs, dim)).astype(np.int8)
    for s in range(seam, n_docs, seam):                        # the same vector on both sides of every seam
        vec[s] = vec[s - 1]
    qvec = rng.integers(-1, 2, (n_q, dim)).astype(np.int8)
    return vec, qvec


@pytest.mark.parametrize("chunk", [256, TILE])
def test_ties_break_by_doc_across_seams(ss_ctx, chunk):
    vec, qvec = ties_world(seam=chunk)
    n_docs, k = vec.shape[0], 10
    sc_all = vm.scores(qvec, vec)
    assert max(np.bincount(sc_all[0] - sc_all[0].min())) >= 200              # hundreds of docs share a score
    straddle = 0
    for q in range(qvec.shape[0]):
        order = np.lexsort((np.arange(n_docs), -sc_all[q].astype(np.int64)))
        straddle += sc_all[q, order[k - 1]] == sc_all[q, order[k]]
    assert straddle >= 1                                                     # a tie across position k: only the doc id decides the row's end
    sc, ti, bi = tiny_scorer(ss_ctx, n_docs)
    try:
        sc.set_doc_vectors(vec)
        ss_ctx.set_option("vec.chunk_docs", chunk)
        for kk in (k, 300):
            got = check_topk(sc, qvec, vec, kk, tag=(chunk, kk))
            for q in range(qvec.shape[0]):
                row = got[0][q]
                same = row["score"][1:] == row["score"][:-1]
                assert (row["doc"][1:][same] > row["doc"][:-1][same]).all()
    finally:
        ss_ctx.set_option("vec.chunk_docs", None)
        close_all(sc, ti, bi)


# ---- chunk seams and merge ----------------------------------------------------------------------------------------------------------

def test_chunk_seams_and_merge(ss_ctx):
    n_docs, dim, k = 1000, 64, 16
    n_chunks = -(-n_docs // TILE)
    rng = np.random.default_rng(9)
    vec = rng.integers(-20, 21, (n_docs, dim)).astype(np.int8)
    qvec = rng.integers(-20, 21, (3, dim)).astype(np.int8)
    qvec[0] = 0
    qvec[0, 0] = 100                                           # query 0 reads position 0 only, query 1 position 1
    qvec[1] = 0
    qvec[1, 1] = 100
    vec[:, 0] = rng.integers(-20, 0, n_docs)
    vec[5 * TILE + 3: 5 * TILE + 3 + k, 0] = np.arange(100, 100 + k)         # case 1: the k best of query 0 in one chunk
    vec[:, 1] = rng.integers(-20, 0, n_docs)
    vec[np.arange(n_chunks) * TILE + 7, 1] = 50 + np.arange(n_chunks)        # case 2: exactly one winner per chunk
    sc_all = vm.scores(qvec, vec)
    assert set(np.argsort(-sc_all[0])[:k] // TILE) == {5}
    assert sorted(np.argsort(-sc_all[1])[:n_chunks] // TILE) == list(range(n_chunks)) and n_chunks == k
    sc, ti, bi = tiny_scorer(ss_ctx, n_docs)
    try:
        sc.set_doc_vectors(vec)
        rows = {}
        for chunk in (None, TILE):
            ss_ctx.set_option("vec.chunk_docs", chunk)
            rows[chunk] = [as_bytes(check_topk(sc, qvec, vec, kk, tag=(chunk, kk))) for kk in (k, 100, 1000)]   # case 3: k above a chunk
        assert rows[None] == rows[TILE]
    finally:
        ss_ctx.set_option("vec.chunk_docs", None)
        close_all(sc, ti, bi)


# ---- masks --------------------------------------------------------------------------------------------------------------------------

def test_masks(ss_ctx):
    n_docs, dim, n_q, k = 1000, 128, 17, 10
    rng = np.random.default_rng(13)
    vec = rng.integers(-128, 128, (n_docs, dim)).astype(np.int8)
    qvec = rng.integers(-128, 128, (n_q, dim)).astype(np.int8)
    best = np.argsort(-vm.scores(qvec[:1], vec)[0], kind="stable")[:2 * k]
    masks = np.zeros((5, n_docs), bool)
    masks[1, 777] = True                                       # one doc
    masks[2] = True
    masks[2, best] = False                                     # without query 0's best 2k docs
    masks[3] = rng.random(n_docs) < 0.3
    masks[3, 3 * TILE:5 * TILE] = False                        # two tiles fully masked out
    masks[4, :TILE] = True                                     # every tile but the first masked out
    sc, ti, bi = tiny_scorer(ss_ctx, n_docs)
    try:
        sc.set_doc_vectors(vec)
        sc.set_doc_masks(engine.pack_doc_masks(masks, n_docs))
        mixed = np.array([2, 0, 1, -1, 3, 4, -1, 0, 3, 1, 2, -1, 4, 3, 0, -1, 2], np.int32)
        for chunk in (None, TILE):
            ss_ctx.set_option("vec.chunk_docs", chunk)
            got = check_topk(sc, qvec, vec, k, mixed, masks, tag=chunk)
            assert got[1][1] == 0 and got[0][1].tobytes() == bytes([FILL]) * (k * 8)         # the empty list: the row is untouched
            assert got[1][2] == 1 and got[0]["doc"][2, 0] == 777
            assert not set(got[0]["doc"][0].tolist()) & set(best.tolist())
            for one in range(5):
                check_topk(sc, qvec, vec, 1000, np.full(n_q, one, np.int32), masks, tag=(chunk, one))
        ss_ctx.set_option("vec.chunk_docs", None)
        # a set built by ss_doc_field_masks, registered as it is
        dates = rng.integers(0, 100, (1, n_docs)).astype(np.int64)
        sc.set_doc_fields(dates)
        words = sc.doc_field_masks(engine.pack_doc_ranges([[(0, 90, 99)]]))
        sc.set_doc_masks(words)
        check_topk(sc, qvec, vec, k, np.zeros(n_q, np.int32), (dates[0] >= 90)[None, :], tag="field mask")
    finally:
        ss_ctx.set_option("vec.chunk_docs", None)
        close_all(sc, ti, bi)


# ---- re-rank and scores -------------------------------------------------------------------------------------------------------------

def test_rerank_and_scores(ss_ctx):
    import torch
    n_docs, dim, n_q, k_in = 500, 128, 5, 40
    rng = np.random.default_rng(17)
    vec = rng.integers(-3, 4, (n_docs, dim)).astype(np.int8)
    vec[:, 8:] = 0                                             # few distinct scores: equal scores inside every window
    qvec = rng.integers(-3, 4, (n_q, dim)).astype(np.int8)
    hits = random_rows(rng, n_q, k_in, n_docs)                 # random bytes in _pad and the scores: carried through
    hits["doc"][:, 3] = hits["doc"][:, 11]                     # a repeated doc
    hits["doc"][:, 5] = n_docs                                 # outside the table
    hits["doc"][:, 20] = 0xFFFFFFFF
    n_hits = np.array([k_in, k_in - 7, 0, 1, k_in], np.int32)
    sc, ti, bi = tiny_scorer(ss_ctx, n_docs)
    try:
        sc.set_doc_vectors(vec)
        want_s = vm.hit_scores(qvec, vec, hits, n_hits, filled((n_q, k_in), np.int32))
        assert (want_s[0] == vm.NO_SCORE).sum() == 2 and len(set(want_s[0].tolist())) < k_in - 5
        got_s = sc.hit_vector_scores(qvec, hits, n_hits, out=filled((n_q, k_in), np.int32))
        assert got_s.tobytes() == want_s.tobytes()
        dev = lambda a: torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).cuda()      # noqa: E731
        d_q, d_hits, d_n = torch.from_numpy(qvec).cuda(), dev(hits), dev(n_hits)
        d_s = dev(filled((n_q, k_in), np.int32))
        sc.hit_vector_scores(d_q, d_hits, d_n, k_in=k_in, out=d_s)
        assert d_s.cpu().numpy().tobytes() == want_s.tobytes()
        for first, k in ((0, k_in), (0, 7), (5, 10), (k_in - 1, 3), (k_in, 3), (k_in + 9, 3), (0, 1024)):
            want = vm.rerank(qvec, vec, hits, n_hits, first, k, filled((n_q, k), engine.HIT_DTYPE), filled(n_q, np.int32),
                             filled((n_q, k), np.int32))
            got = sc.rerank_hits_by_vector(qvec, hits, n_hits, k, first=first,
                                           out=(filled((n_q, k), engine.HIT_DTYPE), filled(n_q, np.int32), filled((n_q, k), np.int32)))
            assert as_bytes(got) == as_bytes(want), (first, k)
            d_out = (dev(filled((n_q, k), engine.HIT_DTYPE)), dev(filled(n_q, np.int32)), dev(filled((n_q, k), np.int32)))
            sc.rerank_hits_by_vector(d_q, d_hits, d_n, k, first=first, k_in=k_in, out=d_out)
            assert [t.cpu().numpy().tobytes() for t in d_out] == as_bytes(want), (first, k)
            got = sc.rerank_hits_by_vector(qvec, hits, n_hits, k, first=first,
                                           out=(filled((n_q, k), engine.HIT_DTYPE), filled(n_q, np.int32), None))
            assert as_bytes(got[:2]) == as_bytes(want[:2])
        # a window of SS_MAX_TOPK rows takes the large sort
        big = random_rows(rng, 2, 1024, n_docs + 50)
        big_n = np.array([1024, 700], np.int32)
        want = vm.rerank(qvec[:2], vec, big, big_n, 3, 1024, filled((2, 1024), engine.HIT_DTYPE), filled(2, np.int32), filled((2, 1024), np.int32))
        got = sc.rerank_hits_by_vector(qvec[:2], big, big_n, 1024, first=3,
                                       out=(filled((2, 1024), engine.HIT_DTYPE), filled(2, np.int32), filled((2, 1024), np.int32)))
        assert as_bytes(got) == as_bytes(want)
        # the device-pointer form of the search gives the host form's bytes
        want_t = vm.topk(qvec, vec, 10, filled((n_q, 10), engine.VEC_HIT_DTYPE), filled(n_q, np.int32))
        d_t = (dev(filled((n_q, 10), engine.VEC_HIT_DTYPE)), dev(filled(n_q, np.int32)))
        sc.vector_topk(d_q, 10, out=d_t)
        assert [t.cpu().numpy().tobytes() for t in d_t] == as_bytes(want_t)
    finally:
        close_all(sc, ti, bi)


# ---- errors -------------------------------------------------------------------------------------------------------------------------

def test_errors_leave_outputs_untouched(ss_ctx):
    n_docs, dim, n_q, k = 200, 64, 4, 5
    rng = np.random.default_rng(23)
    vec = rng.integers(-128, 128, (n_docs, dim)).astype(np.int8)
    qvec = rng.integers(-128, 128, (n_q, dim)).astype(np.int8)
    hits = random_rows(rng, n_q, k, n_docs)
    n_hits = np.full(n_q, k, np.int32)
    lib = ss_ctx.lib
    ptr = lambda a: None if a is None else a.ctypes.data        # noqa: E731
    sc, ti, bi = tiny_scorer(ss_ctx, n_docs)
    try:
        q_ptr, q_terms = np.array([0, 1], np.uint32), np.array([0], np.uint32)
        before = as_bytes(sc.score_topk(q_ptr, q_terms, 3))
        o_t, o_n = filled((n_q, k), engine.VEC_HIT_DTYPE), filled(n_q, np.int32)
        o_s, o_h = filled((n_q, k), np.int32), filled((n_q, k), engine.HIT_DTYPE)
        outs = (o_t, o_n, o_s, o_h)
        clean = as_bytes(outs)
        topk = lambda nq=n_q, q=qvec, m=None, kk=k, h=o_t, n=o_n: lib.ss_vector_topk(sc.h, nq, ptr(q), ptr(m), kk, ptr(h), ptr(n))   # noqa: E731
        scores = lambda nq=n_q, q=qvec, ki=k, h=hits, n=n_hits, o=o_s: lib.ss_hit_vector_scores(sc.h, nq, ptr(q), ki, ptr(h), ptr(n), ptr(o))   # noqa: E731
        rerank = lambda nq=n_q, q=qvec, ki=k, h=hits, n=n_hits, first=0, kk=k, oh=o_h, on=o_n, os_=o_s: lib.ss_rerank_hits_by_vector(   # noqa: E731
            sc.h, nq, ptr(q), ki, ptr(h), ptr(n), first, kk, ptr(oh), ptr(on), ptr(os_))

        def no_table():
            assert topk() == ERR_STATE and scores() == ERR_STATE and rerank() == ERR_STATE
            with pytest.raises(SpaghettiError) as ei:
                sc.vector_topk(qvec, k)
            assert ei.value.code == ERR_STATE
        no_table()
        for bad_dim in (-64, 1, 32, 63, 65, 96, 1088, 2048):
            assert lib.ss_scorer_set_doc_vectors(sc.h, bad_dim, ptr(vec)) == ERR_INVALID, bad_dim
        no_table()
        sc.set_doc_vectors(vec)
        sc.set_doc_masks(engine.pack_doc_masks(np.ones((2, n_docs), bool), n_docs))
        assert lib.ss_scorer_set_doc_vectors(sc.h, 96, ptr(vec)) == ERR_INVALID      # a failing call leaves the table in place
        assert topk() == 0 and scores() == 0 and rerank() == 0
        o_t[:], o_n[:], o_s[:], o_h[:] = filled(o_t.shape, o_t.dtype), filled(n_q, np.int32), filled(o_s.shape, np.int32), filled(o_h.shape, o_h.dtype)
        assert as_bytes(outs) == clean
        for rc, call in ((ERR_INVALID, lambda: lib.ss_vector_topk(None, n_q, ptr(qvec), None, k, ptr(o_t), ptr(o_n))),
                         (ERR_INVALID, lambda: topk(nq=-1)), (ERR_INVALID, lambda: topk(q=None)), (ERR_INVALID, lambda: topk(h=None)),
                         (ERR_INVALID, lambda: topk(n=None)), (ERR_INVALID, lambda: topk(kk=0)), (ERR_INVALID, lambda: topk(kk=-3)),
                         (ERR_UNSUPPORTED, lambda: topk(kk=1025)),
                         (ERR_INVALID, lambda: topk(m=np.array([0, -2, 0, 0], np.int32))),
                         (ERR_INVALID, lambda: topk(m=np.array([0, 1, 2, 0], np.int32))),
                         (ERR_INVALID, lambda: lib.ss_hit_vector_scores(None, n_q, ptr(qvec), k, ptr(hits), ptr(n_hits), ptr(o_s))),
                         (ERR_INVALID, lambda: scores(nq=-1)), (ERR_INVALID, lambda: scores(ki=0)), (ERR_UNSUPPORTED, lambda: scores(ki=1025)),
                         (ERR_INVALID, lambda: scores(q=None)), (ERR_INVALID, lambda: scores(h=None)), (ERR_INVALID, lambda: scores(n=None)),
                         (ERR_INVALID, lambda: scores(o=None)), (ERR_INVALID, lambda: scores(n=np.array([k, k + 1, 0, 0], np.int32))),
                         (ERR_INVALID, lambda: scores(n=np.array([k, -1, 0, 0], np.int32))),
                         (ERR_INVALID, lambda: rerank(nq=-1)), (ERR_INVALID, lambda: rerank(ki=0)), (ERR_INVALID, lambda: rerank(kk=0)),
                         (ERR_INVALID, lambda: rerank(first=-1)), (ERR_UNSUPPORTED, lambda: rerank(ki=1025)),
                         (ERR_UNSUPPORTED, lambda: rerank(kk=1025)), (ERR_INVALID, lambda: rerank(q=None)), (ERR_INVALID, lambda: rerank(h=None)),
                         (ERR_INVALID, lambda: rerank(n=None)), (ERR_INVALID, lambda: rerank(oh=None)), (ERR_INVALID, lambda: rerank(on=None)),
                         (ERR_INVALID, lambda: rerank(n=np.array([k + 1, 0, 0, 0], np.int32)))):
            assert call() == rc
            assert as_bytes(outs) == clean
        both = filled((n_q, 2 * k), engine.HIT_DTYPE)
        assert lib.ss_rerank_hits_by_vector(sc.h, n_q, ptr(qvec), k, ptr(both), ptr(n_hits), 0, k, both.ctypes.data + 40, ptr(o_n), None) == ERR_INVALID
        assert as_bytes(outs) == clean and both.tobytes() == bytes([FILL]) * both.nbytes
        assert topk(nq=0) == 0 and scores(nq=0) == 0 and rerank(nq=0) == 0 and as_bytes(outs) == clean
        assert rerank(os_=None) == 0                                                  # scores_out is optional
        # the lexical call is what it was
        assert as_bytes(sc.score_topk(q_ptr, q_terms, 3)) == before
        sc.set_doc_vectors(None)
        o_h[:], o_n[:] = filled(o_h.shape, o_h.dtype), filled(n_q, np.int32)
        no_table()
        assert as_bytes(outs) == clean
        assert as_bytes(sc.score_topk(q_ptr, q_terms, 3)) == before
    finally:
        close_all(sc, ti, bi)
