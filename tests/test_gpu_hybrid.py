"""GPU parity: hybrid search (ss_score_docs, ss_fuse_hits, ss_hybrid_topk) vs the numpy restatement of the header's definitions
(tests/hybrid_model.py).  Every comparison is equality of bytes: tobytes() on whole output arrays that start from 0xA5 bytes, so an
entry a call must not write is checked with the ones it must.  The lexical tables are a synthetic 1000-doc index built as
tests/test_gpu_score.py builds its own (where ss_score_topk is byte-equal to the oracle: sums of a few float32 weights are exact in
float64 in any order); a 3000-doc one serves the lists whose union reaches 2048."""
import ctypes

import numpy as np
import pytest

from spaghettisearch_amd import SpaghettiError, _lib, engine
from tests import hybrid_model as hm
from tests import vector_model as vm
from tests.test_gpu_collapse import FILL, as_bytes, filled, random_rows
from tests.test_gpu_score import build_weighted, close_all, make_scorer

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE, ERR_UNSUPPORTED = 1, 6, 7
UNKNOWN = 0xFFFFFFFF
RRF, WEIGHTED = engine.FUSE_RRF, engine.FUSE_WEIGHTED


def make_world(oracle, n_docs, dim, seed):
    title, body, mt, mb = build_weighted(oracle, n_docs, 200, 12 * n_docs, 3 * n_docs // 2, seed=seed)
    rng = np.random.default_rng(seed)
    return {"n_docs": n_docs, "n_terms": 200, "title": title, "body": body, "mt": mt, "mb": mb, "prior": None, "dim": dim,
            "vec": rng.integers(-128, 128, (n_docs, dim)).astype(np.int8)}


@pytest.fixture(scope="module")
def world(oracle):
    return make_world(oracle, 1000, 64, 1000)


@pytest.fixture(scope="module")
def world_big(oracle):
    return make_world(oracle, 3000, 192, 3000)


def open_scorer(ss_ctx, w):
    ss_ctx.set_option("vec.chunk_docs", 64)
    sc, ti, bi = make_scorer(ss_ctx, w["n_docs"], w["title"], w["body"], w["mt"], w["mb"])
    sc.set_doc_vectors(w["vec"])
    return sc, ti, bi


@pytest.fixture()
def scorer(ss_ctx, world):
    h = open_scorer(ss_ctx, world)
    yield h
    close_all(*h)
    ss_ctx.set_option("vec.chunk_docs", None)


@pytest.fixture()
def scorer_big(ss_ctx, world_big):
    h = open_scorer(ss_ctx, world_big)
    yield h
    close_all(*h)
    ss_ctx.set_option("vec.chunk_docs", None)


def queries(rows):
    q_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint32)
    return q_ptr, np.array([t for r in rows for t in r], dtype=np.uint32)


def the_queries(w):
    """a 1-token, a 3-token and a 64-token (SS_MAX_QUERY_TERMS) query, a repeated token, an unknown term, an empty term list"""
    return queries([[3], [0, 1, 2], list(range(100, 164)), [5, 7, 5, 5], [UNKNOWN, 9, w["n_terms"] + 2], []])


def fuse_outputs(n_q, k):
    return filled((n_q, k), engine.HIT_DTYPE), filled(n_q, np.int32), filled((n_q, k), engine.FUSED_DTYPE), filled(n_q, np.int32)


# ---- ss_score_docs --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_prior", [False, True])
def test_score_docs_every_doc(world, scorer, with_prior):
    sc = scorer[0]
    n_docs = world["n_docs"]
    q_ptr, q_terms = the_queries(world)
    n_q = len(q_ptr) - 1
    rng = np.random.default_rng(5)
    w, probs = dict(world), None
    if with_prior:
        rank = rng.random((3, n_docs))
        sc.set_prior(rank)
        w["prior"], probs = np.ascontiguousarray(rank.T), rng.random((n_q, 3))
    qlen = np.array([1, 5, 64, 4, 3, 0], np.int32)
    docs = np.tile(np.arange(n_docs, dtype=np.uint32), (n_q, 1))
    n_in = np.full(n_q, n_docs, np.int32)
    for ql in (None, qlen):
        got = sc.score_docs(q_ptr, q_terms, docs, n_in, query_len=ql, topic_probs=probs, out=filled((n_q, n_docs), engine.HIT_DTYPE))
        want = hm.score_docs(w, q_ptr, q_terms, docs, n_in, filled((n_q, n_docs), engine.HIT_DTYPE), query_len=ql, topic_probs=probs)
        for q in range(n_q):
            assert got[q].tobytes() == want[q].tobytes(), (q, ql is None)
        # the rows the ranking itself returns are these rows
        top, n_top = sc.score_topk(q_ptr, q_terms, 100, query_len=ql, topic_probs=probs)
        assert n_top[:5].min() > 0 and n_top[5] == 0
        for q in range(n_q):
            n = int(n_top[q])
            assert top[q, :n].tobytes() == got[q, top["doc"][q, :n].astype(np.int64)].tobytes(), q
    assert (got["title"] != 0).any() and (got["body"] != 0).any() and (got["final"][0] == 0).any() == (not with_prior)


def test_score_docs_edges(world, scorer):
    sc = scorer[0]
    n_docs = world["n_docs"]
    q_ptr, q_terms = the_queries(world)
    n_q = len(q_ptr) - 1
    rng = np.random.default_rng(6)
    for k_in in (1, 37, 1024):
        docs = rng.integers(0, n_docs, (n_q, k_in)).astype(np.uint32)
        docs[:, k_in // 2] = [n_docs, n_docs + 1, 0xFFFFFFFF, 0x80000000, n_docs - 1, 0][:n_q]      # ids at and above n_docs
        n_in = np.array([k_in, 0, k_in, k_in // 2, 1, k_in], np.int32)
        got = sc.score_docs(q_ptr, q_terms, docs, n_in, out=filled((n_q, k_in), engine.HIT_DTYPE))
        want = hm.score_docs(world, q_ptr, q_terms, docs, n_in, filled((n_q, k_in), engine.HIT_DTYPE))
        assert got.tobytes() == want.tobytes(), k_in
        assert got[0, k_in // 2].tobytes() == np.array([(n_docs, 0, 0, 0, 0, 0)], engine.HIT_DTYPE).tobytes()
    assert sc.score_docs(q_ptr, q_terms, docs).tobytes() == hm.score_docs(world, q_ptr, q_terms, docs, np.full(n_q, 1024), np.zeros((n_q, 1024), engine.HIT_DTYPE)).tobytes()


# ---- ss_fuse_hits ---------------------------------------------------------------------------------------------------------------------

def check_fuse(sc, w, q_ptr, q_terms, qvec, lex, n_lex, vec, n_vec, fp, first, k, tag=None, **kw):
    mode, c, w_lex, w_vec = fp
    got = sc.fuse_hits(q_ptr, q_terms, qvec, lex, n_lex, vec, n_vec, k, mode=mode, rrf_c=c, w_lex=w_lex, w_vec=w_vec, first=first,
                       out=fuse_outputs(lex.shape[0], k), **kw)
    want = hm.fuse(w, w["vec"], q_ptr, q_terms, qvec, lex, n_lex, vec, n_vec, fp, first, k, *fuse_outputs(lex.shape[0], k), **kw)
    assert got[1].tolist() == want[1].tolist() and got[3].tolist() == want[3].tolist(), (tag, fp, first, k)
    assert as_bytes(got) == as_bytes(want), (tag, fp, first, k)
    return got


def random_lists(rng, n_q, k_lex, k_vec, n_docs, kind="random"):
    """lex rows of random BYTES (NaN, -0.0, anything in _pad and the scores), vec rows of random scores"""
    lex = random_rows(rng, n_q, k_lex, n_docs)
    vec = np.zeros((n_q, k_vec), engine.VEC_HIT_DTYPE)
    vec["score"] = rng.integers(-2 ** 24, 2 ** 24, (n_q, k_vec))
    vec["doc"] = rng.integers(0, n_docs, (n_q, k_vec))
    if kind == "disjoint":
        for q in range(n_q):
            perm = rng.permutation(n_docs)[:k_lex + k_vec]
            lex["doc"][q], vec["doc"][q] = perm[:k_lex], perm[k_lex:]
    elif kind == "identical":
        for q in range(n_q):
            perm = rng.permutation(n_docs)[:k_lex]
            lex["doc"][q], vec["doc"][q] = perm, perm[::-1]
    return lex, vec


SHAPES = [(1, 1, "random"), (7, 100, "random"), (100, 7, "random"), (1024, 1024, "disjoint"), (1024, 1024, "identical")]


@pytest.mark.parametrize("mode", [RRF, WEIGHTED])
@pytest.mark.parametrize("k_lex,k_vec,kind", SHAPES)
def test_fuse_shapes(world_big, scorer_big, k_lex, k_vec, kind, mode):
    sc, w = scorer_big[0], world_big
    rng = np.random.default_rng(k_lex * 3 + k_vec + mode)
    q_ptr, q_terms = queries([[0, 1, 2], [UNKNOWN], [4, 4]])
    n_q = 3
    qvec = rng.integers(-128, 128, (n_q, w["dim"])).astype(np.int8)
    lex, vec = random_lists(rng, n_q, k_lex, k_vec, 40 if kind == "random" and k_lex > 1 else w["n_docs"], kind)
    n_lex, n_vec = np.array([k_lex, k_lex, k_lex // 2], np.int32), np.array([k_vec, k_vec // 2, k_vec], np.int32)
    fp = (mode, 60, 1.0, 0.5)
    got = check_fuse(sc, w, q_ptr, q_terms, qvec, lex, n_lex, vec, n_vec, fp, 0, 1024, tag=kind)
    if kind == "disjoint":
        assert got[3].tolist() == [2048, 1536, 1536] and got[1].tolist() == [1024] * 3
        check_fuse(sc, w, q_ptr, q_terms, qvec, lex, n_lex, vec, n_vec, fp, 1024, 1024, tag=kind)      # the second half of the largest sort
        check_fuse(sc, w, q_ptr, q_terms, qvec, lex, n_lex, vec, n_vec, fp, 2040, 100, tag=kind)
    if kind == "identical":
        assert got[3].tolist() == [1024, 1024, 1024]
    check_fuse(sc, w, q_ptr, q_terms, qvec, lex, n_lex, vec, n_vec, (mode, 1, -1.0, 2.0), 1, 5, tag=kind)


def special_lists(w):
    """one query per special list -> lex, n_lex, vec, n_vec (k_lex = 8, k_vec = 6)"""
    n_docs = w["n_docs"]
    lex = np.zeros((8, 8), engine.HIT_DTYPE)
    vec = np.zeros((8, 6), engine.VEC_HIT_DTYPE)
    lex["final"] = np.arange(64).reshape(8, 8) * 0.25 + 1
    lex["_pad"] = 77                                              # given rows come back as given
    vec["score"] = 1000 - np.arange(48).reshape(8, 6) * 13
    lex["doc"] = (np.arange(64).reshape(8, 8) * 7) % 50
    vec["doc"] = (np.arange(48).reshape(8, 6) * 11 + 3) % 50
    n_lex = np.array([0, 8, 0, 8, 8, 8, 8, 8], np.int32)         # 0: empty lexical, 1: empty vector, 2: both empty
    n_vec = np.array([6, 0, 0, 6, 6, 6, 6, 6], np.int32)
    lex["doc"][3] = [5, 5, 9, 5, 9, 2, 2, 5]                      # 3: duplicated docs within both lists
    vec["doc"][3] = [9, 9, 9, 1, 1, 5]
    lex["doc"][4] = [4, n_docs, 6, 0xFFFFFFFF, 8, n_docs + 7, 10, 12]      # 4: invalid ids in the middle: later ranks stay positional
    vec["doc"][4] = [8, 0x80000000, 4, n_docs, 30, 31]
    lex["doc"][5] = [20, 21, 22, 23, 24, 25, 26, 27]              # 5: a NaN, an infinite and a negative-zero final
    lex["final"][5] = [np.nan, np.inf, -0.0, 0.0, -np.inf, 1.0, np.nan, -1.0]
    vec["doc"][5] = [40, 41, 22, 20, 42, 43]                      # 40 .. 43: vector-only candidates beside them
    return lex, n_lex, vec, n_vec


def test_fuse_special_lists_parameters_and_paging(world, scorer):
    sc, w = scorer[0], dict(world)
    # every vector-only candidate of row 5 has final 0.0 when the query matches nothing: the tie with -0.0 at w_vec = 0
    q_ptr, q_terms = queries([[0, 1], [2], [3], [0, 5], [1, 1], [UNKNOWN], [7, 8, 9], [10]])
    rng = np.random.default_rng(9)
    qvec = rng.integers(-128, 128, (8, w["dim"])).astype(np.int8)
    lex, n_lex, vec, n_vec = special_lists(w)
    fps = [(RRF, 1, 1.0, 1.0), (RRF, 60, 1.0, 1.0), (RRF, 60, 0.0, 1.0), (RRF, 60, 1.0, 0.0), (RRF, 1, -1.0, -2.5),
           (WEIGHTED, 60, 1.0, 0.0), (WEIGHTED, 60, 0.0, 1.0), (WEIGHTED, 1, 1.0, 1e-3), (WEIGHTED, 60, -1.0, -1e-3), (WEIGHTED, 60, 0.0, 0.0)]
    for fp in fps:
        got = check_fuse(sc, w, q_ptr, q_terms, qvec, lex, n_lex, vec, n_vec, fp, 0, 20, tag="special")
    assert got[3].tolist()[:3] == [6, 8, 0] and got[1].tolist()[2] == 0
    got = check_fuse(sc, w, q_ptr, q_terms, qvec, lex, n_lex, vec, n_vec, (WEIGHTED, 60, 1.0, 0.0), 0, 20)
    row = got[0][5][:int(got[1][5])]
    assert row["doc"].tolist()[:1] == [21] and set(row["doc"][-2:].tolist()) == {20, 26}                 # +inf first, the NaN finals last
    zeros = [int(d) for d, f in zip(row["doc"], got[2][5]["score"]) if f == 0]
    assert zeros == [22, 23, 40, 41, 42, 43]                     # -0.0 ties 0.0: by doc
    n_union = int(got[3][3])
    for first, k in ((0, 1), (2, 3), (n_union, 4), (n_union + 5, 4), (0, 1024), (1, 1024), (5000, 1)):
        check_fuse(sc, w, q_ptr, q_terms, qvec, lex, n_lex, vec, n_vec, (RRF, 60, 1.0, 1.0), first, k, tag="paging")
    # with a prior and query lengths the completed rows change, the given ones do not
    rank = rng.random((2, w["n_docs"]))
    sc.set_prior(rank)
    w["prior"] = np.ascontiguousarray(rank.T)
    check_fuse(sc, w, q_ptr, q_terms, qvec, lex, n_lex, vec, n_vec, (WEIGHTED, 60, 1.0, 1e-4), 0, 20, tag="prior",
               query_len=np.arange(8, dtype=np.int32), topic_probs=rng.random((8, 2)))


# ---- ss_hybrid_topk -------------------------------------------------------------------------------------------------------------------

def hybrid_case(world, sc, variant, rng):
    n_docs = world["n_docs"]
    q_ptr, q_terms = the_queries(world)
    n_q = len(q_ptr) - 1
    w = dict(world)
    mask_id = masks = probs = None
    if variant in ("all-open", "mix"):
        masks = rng.random((4, n_docs)) < 0.3
        masks[2] = False                                         # allows no doc
        masks[3] = False
        masks[3, 617] = True                                     # allows one doc
        sc.set_doc_masks(engine.pack_doc_masks(masks, n_docs))
        mask_id = np.full(n_q, -1, np.int32) if variant == "all-open" else np.array([0, 2, 3, -1, 1, 3], np.int32)
    if variant == "prior":
        rank = rng.random((3, n_docs))
        sc.set_prior(rank)
        w["prior"], probs = np.ascontiguousarray(rank.T), rng.random((n_q, 3))
    qvec = rng.integers(-128, 128, (n_q, world["dim"])).astype(np.int8)
    return w, q_ptr, q_terms, qvec, mask_id, masks, probs


@pytest.mark.parametrize("k_window", [1, 10, 1024])
@pytest.mark.parametrize("variant", ["plain", "all-open", "mix", "prior"])
def test_hybrid_equals_its_two_calls_and_the_fusion(world, scorer, k_window, variant):
    sc = scorer[0]
    rng = np.random.default_rng(k_window)
    w, q_ptr, q_terms, qvec, mask_id, masks, probs = hybrid_case(world, sc, variant, rng)
    n_q = len(q_ptr) - 1
    lex, n_lex = sc.score_topk_masked(q_ptr, q_terms, mask_id, k_window, topic_probs=probs)
    vec, n_vec = sc.vector_topk(qvec, k_window, mask_id)
    for fp, first, k in (((RRF, 60, 1.0, 1.0), 0, 20), ((WEIGHTED, 60, 1.0, 1e-3), 0, 1024), ((RRF, 1, 2.0, 1.0), 3, 7)):
        mode, c, w_lex, w_vec = fp
        got = sc.hybrid_topk(q_ptr, q_terms, qvec, k_window, k, mode=mode, rrf_c=c, w_lex=w_lex, w_vec=w_vec, first=first, mask_id=mask_id,
                             topic_probs=probs, out=fuse_outputs(n_q, k))
        want = hm.hybrid(w, w["vec"], q_ptr, q_terms, qvec, lex, n_lex, k_window, fp, first, k, *fuse_outputs(n_q, k), mask_id=mask_id,
                         masks=masks, topic_probs=probs)
        assert as_bytes(got) == as_bytes(want), (fp, first, k)
        two = sc.fuse_hits(q_ptr, q_terms, qvec, lex, n_lex, vec, n_vec, k, mode=mode, rrf_c=c, w_lex=w_lex, w_vec=w_vec, first=first,
                           topic_probs=probs, out=fuse_outputs(n_q, k))
        assert as_bytes(got) == as_bytes(two), (fp, first, k)
    if variant == "mix":
        assert int(got[3][1]) == 0 and int(got[3][2]) == 1       # the mask of no doc, the mask of one
    if variant == "plain" and k_window == 10:
        assert (got[2]["lex_rank"][0, :int(got[1][0])] == 0).any() and (got[2]["vec_rank"][0, :int(got[1][0])] == 0).any()


def test_hybrid_device_outputs_seven_calls_back_to_back(ss_ctx, world, scorer):
    """seven calls into device buffers of their own, more than twice the scorer's turns, alternating between two batches; one
    synchronise at the end; the bytes of each are the host call's"""
    import torch
    sc, lib = scorer[0], ss_ctx.lib
    rng = np.random.default_rng(12)
    q_ptr, q_terms = the_queries(world)
    qp2, qt2 = queries([[1, 2], [60, 61, 62], [8]])
    k_window, k = 50, 30
    fp = _lib.SsFuseParams(WEIGHTED, 60, 1.0, 1e-3)
    rounds = []
    for r in range(7):
        qp, qt = (q_ptr, q_terms) if r % 2 == 0 else (qp2, qt2)
        nq = len(qp) - 1
        qv = rng.integers(-128, 128, (nq, world["dim"])).astype(np.int8)
        rounds.append({"qp": qp, "qt": qt, "nq": nq, "qv": qv, "d_qv": torch.from_numpy(qv).cuda(), "first": r,
                       "out": [torch.full((n,), FILL, dtype=torch.uint8, device="cuda") for n in (nq * k * 40, nq * 4, nq * k * 16, nq * 4)]})
    torch.cuda.synchronize()
    for c in rounds:
        rc = lib.ss_hybrid_topk(sc.h, c["nq"], c["qp"].ctypes.data, c["qt"].ctypes.data, None, None, c["d_qv"].data_ptr(), None, k_window,
                                ctypes.byref(fp), c["first"], k, *[t.data_ptr() for t in c["out"]])
        assert rc == 0
    ss_ctx.synchronize()
    for r, c in enumerate(rounds):
        ref = sc.hybrid_topk(c["qp"], c["qt"], c["qv"], k_window, k, mode=WEIGHTED, w_vec=1e-3, first=c["first"], out=fuse_outputs(c["nq"], k))
        assert [t.cpu().numpy().tobytes() for t in c["out"]] == as_bytes(ref), r
    assert any(int(c["out"][1].view(torch.int32).sum()) > 0 for c in rounds)


# ---- pointer placements ---------------------------------------------------------------------------------------------------------------

def test_pointer_placements(ss_ctx, world, scorer):
    import torch
    sc, lib, w = scorer[0], ss_ctx.lib, world
    rng = np.random.default_rng(4)
    q_ptr, q_terms = the_queries(w)
    n_q, k_lex, k_vec, first, k = len(q_ptr) - 1, 130, 70, 3, 40
    qvec = rng.integers(-128, 128, (n_q, w["dim"])).astype(np.int8)
    lex, vec = random_lists(rng, n_q, k_lex, k_vec, 150)
    lex["doc"][:, 5] = w["n_docs"] + 3
    n_lex = rng.integers(0, k_lex + 1, n_q).astype(np.int32)
    n_vec = rng.integers(0, k_vec + 1, n_q).astype(np.int32)
    fpt = (WEIGHTED, 60, 1.0, 1e-3)
    fp = _lib.SsFuseParams(*fpt)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()

    ptr = lambda a: None if a is None else a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data       # noqa: E731
    back = lambda o: [None if a is None else (a.cpu().numpy() if hasattr(a, "cpu") else a).tobytes() for a in o]      # noqa: E731

    def run(ins, o, code=0):
        torch.cuda.synchronize()
        rc = lib.ss_fuse_hits(sc.h, n_q, q_ptr.ctypes.data, q_terms.ctypes.data, None, None, ptr(ins[0]), k_lex, ptr(ins[1]), ptr(ins[2]),
                              k_vec, ptr(ins[3]), ptr(ins[4]), ctypes.byref(fp), first, k, ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(o[3]))
        assert rc == code
        ss_ctx.synchronize()
        return back(o)

    ref = as_bytes(hm.fuse(w, w["vec"], q_ptr, q_terms, qvec, lex, n_lex, vec, n_vec, fpt, first, k, *fuse_outputs(n_q, k)))
    h_in = [qvec, lex, n_lex, vec, n_vec]
    d_in = [dev(a) for a in h_in]
    host_out = lambda: list(fuse_outputs(n_q, k))                              # noqa: E731
    dev_out = lambda: [dev(a) for a in fuse_outputs(n_q, k)]                  # noqa: E731
    assert run(d_in, dev_out()) == ref                                         # every array in device memory
    assert run(h_in, host_out()) == ref                                        # every array in host memory
    for i in range(5):                                                         # each input alone in the other memory
        assert run([d_in[j] if j == i else h_in[j] for j in range(5)], host_out()) == ref, i
        assert run([h_in[j] if j == i else d_in[j] for j in range(5)], dev_out()) == ref, i
    for i in range(4):                                                         # each output alone in the other memory
        o = host_out()
        o[i] = dev(o[i])
        assert run(h_in, o) == ref, i
        o = dev_out()
        o[i] = fuse_outputs(n_q, k)[i]
        assert run(d_in, o) == ref, i
    for drop in ((2,), (3,), (2, 3)):                                          # fused_out / n_union_out NULL
        for make, ins in ((host_out, h_in), (dev_out, d_in)):
            o = make()
            for i in drop:
                o[i] = None
            assert run(ins, o) == [None if i in drop else ref[i] for i in range(4)]
    # device counts outside their range are clamped by the kernel; the same arrays in host memory are refused
    bad_l, bad_v = n_lex.copy(), n_vec.copy()
    bad_l[0], bad_l[1], bad_v[2], bad_v[3] = -1, k_lex + 5, -2 ** 31, k_vec + 1
    clamped = as_bytes(hm.fuse(w, w["vec"], q_ptr, q_terms, qvec, lex, bad_l, vec, bad_v, fpt, first, k, *fuse_outputs(n_q, k), clamp=True))
    assert run([d_in[0], d_in[1], dev(bad_l), d_in[3], dev(bad_v)], dev_out()) == clamped
    assert run([qvec, lex, dev(bad_l), vec, dev(bad_v)], host_out()) == clamped
    untouched = as_bytes(fuse_outputs(n_q, k))
    assert run([qvec, lex, bad_l, vec, n_vec], host_out(), code=ERR_INVALID) == untouched
    assert run([qvec, lex, n_lex, vec, bad_v], host_out(), code=ERR_INVALID) == untouched
    # ss_score_docs: docs, n_in and hits_out, each in either memory
    docs = rng.integers(0, w["n_docs"] + 4, (n_q, k_lex)).astype(np.uint32)
    want = hm.score_docs(w, q_ptr, q_terms, docs, n_lex, filled((n_q, k_lex), engine.HIT_DTYPE)).tobytes()
    want_c = hm.score_docs(w, q_ptr, q_terms, docs, bad_l, filled((n_q, k_lex), engine.HIT_DTYPE), clamp=True).tobytes()

    def run_sd(d, n, o, code=0):
        torch.cuda.synchronize()
        rc = lib.ss_score_docs(sc.h, n_q, q_ptr.ctypes.data, q_terms.ctypes.data, None, None, k_lex, ptr(d), ptr(n), ptr(o))
        assert rc == code
        ss_ctx.synchronize()
        return back([o])[0]

    new = lambda: filled((n_q, k_lex), engine.HIT_DTYPE)                       # noqa: E731
    for d in (docs, dev(docs)):
        for n in (n_lex, dev(n_lex)):
            for o in (new(), dev(new())):
                assert run_sd(d, n, o) == want
    assert run_sd(dev(docs), dev(bad_l), dev(new())) == want_c and run_sd(docs, dev(bad_l), new()) == want_c
    assert run_sd(docs, bad_l, new(), code=ERR_INVALID) == new().tobytes()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_outputs_untouched(ss_ctx, world):
    sc, ti, bi = make_scorer(ss_ctx, world["n_docs"], world["title"], world["body"], world["mt"], world["mb"])
    try:
        lib = ss_ctx.lib
        rng = np.random.default_rng(8)
        q_ptr, q_terms = queries([[0], [1, 2]])
        qvec = rng.integers(-128, 128, (2, world["dim"])).astype(np.int8)
        lex, vec = random_lists(rng, 2, 4, 5, world["n_docs"])
        n_lex, n_vec = np.array([4, 2], np.int32), np.array([5, 0], np.int32)
        docs = np.array([[1, 2, 3], [4, 5, 6]], np.uint32)
        n_in = np.array([3, 1], np.int32)
        out = fuse_outputs(2, 3)
        untouched = as_bytes(fuse_outputs(2, 3))
        ptr = lambda a: None if a is None else a.ctypes.data       # noqa: E731
        good = _lib.SsFuseParams(RRF, 60, 1.0, 1.0)

        def fuse(code, handle="sc", n_q=2, qp=q_ptr, qv=qvec, k_lex=4, lx=lex, nl=n_lex, k_vec=5, vc=vec, nv=n_vec, fp=good, first=0, k=3,
                 o0=out[0], o1=out[1]):
            rc = lib.ss_fuse_hits(sc.h if handle == "sc" else handle, n_q, ptr(qp), ptr(q_terms), None, None, ptr(qv), k_lex, ptr(lx), ptr(nl),
                                  k_vec, ptr(vc), ptr(nv), None if fp is None else ctypes.byref(fp), first, k, ptr(o0), ptr(o1), ptr(out[2]),
                                  ptr(out[3]))
            assert rc == code, (rc, code)
            assert as_bytes(out) == untouched

        def hybrid(code, handle="sc", n_q=2, qp=q_ptr, qv=qvec, k_window=4, fp=good, first=0, k=3, o0=out[0], o1=out[1], mask=None, probs=None):
            rc = lib.ss_hybrid_topk(sc.h if handle == "sc" else handle, n_q, ptr(qp), ptr(q_terms), None, ptr(probs), ptr(qv), ptr(mask),
                                    k_window, None if fp is None else ctypes.byref(fp), first, k, ptr(o0), ptr(o1), ptr(out[2]), ptr(out[3]))
            assert rc == code, (rc, code)
            assert as_bytes(out) == untouched

        def sdocs(code, handle="sc", n_q=2, qp=q_ptr, k_in=3, d=docs, n=n_in, o=out[0]):
            rc = lib.ss_score_docs(sc.h if handle == "sc" else handle, n_q, ptr(qp), ptr(q_terms), None, None, k_in, ptr(d), ptr(n), ptr(o))
            assert rc == code, (rc, code)
            assert as_bytes(out) == untouched
        # no vector table yet
        fuse(ERR_STATE)
        hybrid(ERR_STATE)
        with pytest.raises(SpaghettiError) as ei:
            sc.hybrid_topk(q_ptr, q_terms, qvec, 4, 3, out=out)
        assert ei.value.code == ERR_STATE and as_bytes(out) == untouched
        sc.set_doc_vectors(world["vec"])
        bad_fps = [_lib.SsFuseParams(2, 60, 1.0, 1.0), _lib.SsFuseParams(-1, 60, 1.0, 1.0), _lib.SsFuseParams(RRF, 0, 1.0, 1.0),
                   _lib.SsFuseParams(WEIGHTED, -3, 1.0, 1.0), _lib.SsFuseParams(RRF, 60, float("inf"), 1.0),
                   _lib.SsFuseParams(RRF, 60, 1.0, float("nan")), _lib.SsFuseParams(WEIGHTED, 60, float("-inf"), 1.0)]
        for fn in (fuse, hybrid):
            fn(ERR_INVALID, handle=None)
            fn(ERR_INVALID, n_q=-1)
            fn(ERR_INVALID, fp=None)
            for fp in bad_fps:
                fn(ERR_INVALID, fp=fp)
            fn(ERR_INVALID, qv=None)
            fn(ERR_INVALID, qp=None)
            fn(ERR_INVALID, qp=np.array([0, 3, 2], np.uint32))
            fn(ERR_INVALID, first=-1)
            fn(ERR_INVALID, k=0)
            fn(ERR_INVALID, o0=None)
            fn(ERR_INVALID, o1=None)
            fn(ERR_UNSUPPORTED, k=1025)
        for name in ("k_lex", "k_vec"):
            fuse(ERR_INVALID, **{name: 0})
            fuse(ERR_UNSUPPORTED, **{name: 1025})
        for name in ("lx", "nl", "vc", "nv"):
            fuse(ERR_INVALID, **{name: None})
        fuse(ERR_INVALID, nl=np.array([5, 1], np.int32))
        fuse(ERR_INVALID, nl=np.array([1, -1], np.int32))
        fuse(ERR_INVALID, nv=np.array([6, 1], np.int32))
        fuse(ERR_INVALID, nv=np.array([1, -1], np.int32))
        hybrid(ERR_INVALID, k_window=0)
        hybrid(ERR_UNSUPPORTED, k_window=1025)
        hybrid(ERR_INVALID, mask=np.array([0, -1], np.int32))                 # no allow-list registered
        hybrid(ERR_STATE, probs=np.ones(2))                                   # topic_probs without a prior
        sdocs(ERR_INVALID, handle=None)
        sdocs(ERR_INVALID, n_q=-1)
        sdocs(ERR_INVALID, qp=None)
        sdocs(ERR_INVALID, qp=np.array([0, 3, 2], np.uint32))
        sdocs(ERR_INVALID, k_in=0)
        sdocs(ERR_UNSUPPORTED, k_in=1025)
        for name in ("d", "n", "o"):
            sdocs(ERR_INVALID, **{name: None})
        sdocs(ERR_INVALID, n=np.array([4, 1], np.int32))
        sdocs(ERR_INVALID, n=np.array([1, -1], np.int32))
        # hits_out overlapping lex: the same array, and one that starts inside it
        both = np.concatenate([lex.reshape(-1), lex.reshape(-1)])
        before = both.tobytes()
        for off in (0, 1, 7):
            rc = lib.ss_fuse_hits(sc.h, 2, ptr(q_ptr), ptr(q_terms), None, None, ptr(qvec), 4, both.ctypes.data, ptr(n_lex), 5, ptr(vec),
                                  ptr(n_vec), ctypes.byref(good), 0, 3, both[off:].ctypes.data, ptr(out[1]), None, None)
            assert rc == ERR_INVALID and both.tobytes() == before and as_bytes(out) == untouched
        fuse(0, n_q=0)                                                        # nothing to do: SS_OK, nothing written
        fuse(0, n_q=0, qv=None, lx=None, nl=None, vc=None, nv=None, o0=None, o1=None)
        hybrid(0, n_q=0, qp=np.array([0], np.uint32))
        sdocs(0, n_q=0)
        # the same arguments untouched are accepted, and after clearing the table refused again
        got = sc.fuse_hits(q_ptr, q_terms, qvec, lex, n_lex, vec, n_vec, 3, out=fuse_outputs(2, 3))
        w = dict(world)
        assert as_bytes(got) == as_bytes(hm.fuse(w, w["vec"], q_ptr, q_terms, qvec, lex, n_lex, vec, n_vec, (RRF, 60, 1.0, 1.0), 0, 3,
                                                 *fuse_outputs(2, 3)))
        sc.set_doc_vectors(None)
        fuse(ERR_STATE)
        hybrid(ERR_STATE)
    finally:
        close_all(sc, ti, bi)


# ---- the neighbours -------------------------------------------------------------------------------------------------------------------

def test_neighbours_return_the_same_bytes_after_the_hybrid_calls(world, scorer):
    """the blocks the window calls share are not left dirty: re-rank, collapse and the scoring call before and after"""
    sc = scorer[0]
    rng = np.random.default_rng(2)
    q_ptr, q_terms = the_queries(world)
    n_q = len(q_ptr) - 1
    qvec = rng.integers(-128, 128, (n_q, world["dim"])).astype(np.int8)
    sc.set_doc_groups((np.arange(world["n_docs"]) % 9).astype(np.uint32))

    def neighbours():
        rows, n_rows = sc.score_topk(q_ptr, q_terms, 100)
        rr = sc.rerank_hits_by_vector(qvec, rows, n_rows, 40, first=2, out=(filled((n_q, 40), engine.HIT_DTYPE), filled(n_q, np.int32),
                                                                             filled((n_q, 40), np.int32)))
        cl = sc.collapse_hits(rows, n_rows, 2, 40, first=1, out=(filled((n_q, 40), engine.HIT_DTYPE), filled(n_q, np.int32),
                                                                 filled((n_q, 40), np.uint32), filled(n_q, np.int32)))
        return as_bytes((rows, n_rows)) + as_bytes(rr) + as_bytes(cl)

    before = neighbours()
    rows, n_rows = sc.score_topk(q_ptr, q_terms, 100)
    vec, n_vec = sc.vector_topk(qvec, 100)
    sc.fuse_hits(q_ptr, q_terms, qvec, rows, n_rows, vec, n_vec, 50)
    sc.hybrid_topk(q_ptr, q_terms, qvec, 100, 50, mode=WEIGHTED, w_vec=1e-3)
    sc.score_docs(q_ptr, q_terms, np.tile(np.arange(1000, dtype=np.uint32), (n_q, 1)))
    assert neighbours() == before
