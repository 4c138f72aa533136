"""GPU parity: vector lists (ss_scorer_set_vector_lists, ss_vector_assign_lists, ss_vector_topk_probed, engine.train_vector_lists) vs the
numpy restatement of the header's definitions (tests/vector_lists_model.py).  Scores are exact 32-bit integers, ties break by doc id
(rows) and by list id (probes), so every comparison is equality: tobytes() on whole output arrays that start from 0xA5 bytes, so an
entry a call must not write is checked with the ones it must."""
import numpy as np
import pytest

from spaghettisearch_amd import SpaghettiError, engine
from tests import vector_lists_model as vlm
from tests import vector_model as vm
from tests.test_gpu_collapse import FILL, as_bytes, filled
from tests.test_gpu_score import close_all
from tests.test_gpu_vector import tiny_scorer

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE, ERR_UNSUPPORTED = 1, 6, 7
TILE = 64
NO_LIST = vlm.NO_LIST


def world(seed, n_docs=1000, dim=64, n_lists=7, n_q=17, lo=-128, hi=128):
    rng = np.random.default_rng(seed)
    vec = rng.integers(lo, hi, (n_docs, dim)).astype(np.int8)
    cent = rng.integers(lo, hi, (n_lists, dim)).astype(np.int8)
    qvec = rng.integers(lo, hi, (n_q, dim)).astype(np.int8)
    return rng, vec, cent, qvec


def check_probed(sc, qvec, vec, cent, lod, k, n_probe, mask_id=None, masks=None, tag=None):
    n_q = qvec.shape[0]
    n_p = min(n_probe, cent.shape[0])
    want = vlm.topk_probed(qvec, vec, cent, lod, k, n_probe, filled((n_q, k), engine.VEC_HIT_DTYPE), filled(n_q, np.int32), mask_id, masks)
    got = sc.vector_topk_probed(qvec, k, n_probe, mask_id, out=(filled((n_q, k), engine.VEC_HIT_DTYPE), filled(n_q, np.int32), filled((n_q, n_p), np.uint32)))
    assert got[2].tolist() == want[2].tolist(), tag
    assert got[1].tolist() == want[1].tolist(), tag
    for q in range(n_q):
        n = int(want[1][q])
        assert got[0][q, :n].tolist() == want[0][q, :n].tolist(), (tag, q)
    assert as_bytes(got) == as_bytes(want), tag
    return got


@pytest.fixture
def seg64(ss_ctx):
    ss_ctx.set_option("vec.list_seg_rows", TILE)
    yield ss_ctx
    for name in ("vec.list_seg_rows", "vec.list_batch_q", "vec.assign_batch", "vec.chunk_docs"):
        ss_ctx.set_option(name, None)


# ---- identity ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [64, 192])
def test_every_list_probed_is_vector_topk(ss_ctx, dim):
    rng, vec, cent, qvec = world(dim, dim=dim)
    lod = vlm.assign(vec, cent)[0]
    sc, ti, bi = tiny_scorer(ss_ctx, vec.shape[0])
    try:
        sc.set_doc_vectors(vec)
        sc.set_vector_lists(cent, lod)
        for k in (10, 100):
            exact = sc.vector_topk(qvec, k, out=(filled((17, k), engine.VEC_HIT_DTYPE), filled(17, np.int32)))
            for n_probe in (7, 1024):
                got = sc.vector_topk_probed(qvec, k, n_probe, out=(filled((17, k), engine.VEC_HIT_DTYPE), filled(17, np.int32)))
                assert as_bytes(got) == as_bytes(exact), (dim, k, n_probe)
                check_probed(sc, qvec, vec, cent, lod, k, n_probe, tag=(dim, k, n_probe))
    finally:
        close_all(sc, ti, bi)


# ---- shapes -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_q", [1, 17, 65, 130])
def test_shapes_all_queries_on_one_list(ss_ctx, n_q):
    """more than 64 queries on one list cross the seam between two query groups of a work item"""
    rng, vec, cent, _ = world(31, dim=128)
    cent[2] = np.where(np.arange(128) % 2 == 0, 120, -120)
    qvec = np.clip(cent[2].astype(np.int32) + rng.integers(-8, 9, (n_q, 128)), -128, 127).astype(np.int8)
    lod = vlm.assign(vec, cent)[0]
    assert (vlm.probes(qvec, cent, 1)[:, 0] == 2).all()
    sc, ti, bi = tiny_scorer(ss_ctx, vec.shape[0])
    try:
        sc.set_doc_vectors(vec)
        sc.set_vector_lists(cent, lod)
        for n_probe in (1, 3):
            for k in (10, 100):
                check_probed(sc, qvec, vec, cent, lod, k, n_probe, tag=(n_q, n_probe, k))
    finally:
        close_all(sc, ti, bi)


def test_shapes_queries_on_disjoint_lists(ss_ctx):
    rng, vec, cent, _ = world(37, dim=64, n_lists=40)
    qvec = cent[np.arange(33) % 40].copy()                     # query q is centroid q: its own list first
    lod = vlm.assign(vec, cent)[0]
    assert len(set(vlm.probes(qvec, cent, 1)[:, 0].tolist())) == 33
    sc, ti, bi = tiny_scorer(ss_ctx, vec.shape[0])
    try:
        sc.set_doc_vectors(vec)
        sc.set_vector_lists(cent, lod)
        for n_probe in (1, 3):
            check_probed(sc, qvec, vec, cent, lod, 10, n_probe, tag=n_probe)
    finally:
        close_all(sc, ti, bi)


# ---- skew and seams ---------------------------------------------------------------------------------------------------------------

def test_skew_and_list_seams(seg64):
    """lists of length 1, 63, 0, 64, 65 and 900 at 64 rows per segment; the rows behind a list's end in the same tile are the next
    list's, and those are built to be the query's best docs: they must not appear"""
    lens = [1, 63, 0, 64, 65, 900, 0]
    n_lists, n_docs, dim = len(lens), sum(lens), 64
    rng = np.random.default_rng(41)
    lod = np.repeat(np.arange(n_lists), lens).astype(np.uint32)
    rng.shuffle(lod)
    vec = rng.integers(-5, 6, (n_docs, dim)).astype(np.int8)
    cent = np.zeros((n_lists, dim), np.int8)
    cent[np.arange(n_lists), np.arange(n_lists)] = 100
    qvec = cent.copy()
    follower = {0: 1, 1: 3, 3: 4, 4: 5}                        # the next list in list-major order that has rows
    for l, nxt in follower.items():
        qvec[l, 20 + l] = 100
        vec[lod == nxt, 20 + l] = 127                          # the follower's docs score highest under query l ...
        vec[lod == l, 20 + l] = rng.integers(-5, 6, lens[l])
    vec[:, :n_lists] = 0                                       # ... and no doc moves a centroid score
    assert vlm.probes(qvec, cent, 1)[:, 0].tolist() == list(range(n_lists))
    best = vm.topk(qvec, vec, 10, np.zeros((n_lists, 10), engine.VEC_HIT_DTYPE), np.zeros(n_lists, np.int32))[0]
    for l, nxt in follower.items():
        assert (lod[best["doc"][l, :min(10, lens[nxt])]] == nxt).all()
    sc, ti, bi = tiny_scorer(seg64, n_docs)
    try:
        sc.set_doc_vectors(vec)
        sc.set_vector_lists(cent, lod)
        for k in (10, 100, 1000):
            got = check_probed(sc, qvec, vec, cent, lod, k, 1, tag=k)
            assert got[1].tolist() == [min(k, n) for n in lens]
            for l in range(n_lists):
                assert (lod[got[0]["doc"][l, :got[1][l]]] == l).all()
        rows = [as_bytes(check_probed(sc, qvec, vec, cent, lod, 100, p, tag=p)) for p in (2, 7)]
        seg64.set_option("vec.list_seg_rows", None)            # one segment per list: the same bytes
        assert [as_bytes(check_probed(sc, qvec, vec, cent, lod, 100, p, tag=p)) for p in (2, 7)] == rows
    finally:
        close_all(sc, ti, bi)


# ---- ties -------------------------------------------------------------------------------------------------------------------------

def test_ties_across_segments_lists_and_centroids(seg64):
    rng, vec, cent, qvec = world(43, n_lists=6, lo=-1, hi=2)
    cent = rng.integers(-128, 128, cent.shape).astype(np.int8)
    cent[4] = cent[1]                                          # equal centroid scores under every query: list 1 before list 4
    cent[5] = cent[0]
    lod = rng.integers(0, 6, 1000).astype(np.uint32)
    vec[500:] = vec[:500]                                      # every vector twice, the twins in any two lists and segments
    sc_all = vm.scores(qvec, vec)
    assert max(np.bincount(sc_all[0] - sc_all[0].min())) >= 50
    pr = vlm.probes(qvec, cent, 6)
    for q in range(17):
        row = pr[q].tolist()
        assert row.index(1) < row.index(4) and row.index(0) < row.index(5)
    sc, ti, bi = tiny_scorer(seg64, 1000)
    try:
        sc.set_doc_vectors(vec)
        sc.set_vector_lists(cent, lod)
        for n_probe in (1, 2, 3, 5):                           # some value cuts every query's row between the twins
            for k in (10, 300):
                got = check_probed(sc, qvec, vec, cent, lod, k, n_probe, tag=(n_probe, k))
                for q in range(17):
                    row = got[0][q, :got[1][q]]
                    same = row["score"][1:] == row["score"][:-1]
                    assert (row["doc"][1:][same] > row["doc"][:-1][same]).all()
        cut = sum(int(1 in pr[q, :p]) != int(4 in pr[q, :p]) for q in range(17) for p in (1, 2, 3, 5))
        assert cut >= 1                                        # only the list id decided which of the tied lists was probed
    finally:
        close_all(sc, ti, bi)


# ---- fewer candidates than k, SS_NO_LIST, masks -----------------------------------------------------------------------------------

def test_fewer_candidates_than_k(ss_ctx):
    rng, vec, cent, qvec = world(47)
    lod = vlm.assign(vec, cent)[0]
    sc, ti, bi = tiny_scorer(ss_ctx, 1000)
    try:
        sc.set_doc_vectors(vec)
        sc.set_vector_lists(cent, lod)
        got = check_probed(sc, qvec, vec, cent, lod, 600, 1, tag="k above the list")
        assert (got[1] < 600).all() and (got[1] > 0).all()
        q, n = 0, int(got[1][0])
        assert got[0][q, n:].tobytes() == bytes([FILL]) * ((600 - n) * 8)          # rows past the count keep the sentinel
    finally:
        close_all(sc, ti, bi)


def test_docs_in_no_list_are_never_returned(ss_ctx):
    rng, vec, cent, qvec = world(53)
    lod = vlm.assign(vec, cent)[0]
    best = np.unique(np.argsort(-vm.scores(qvec, vec), axis=1, kind="stable")[:, :5])
    lod[best] = NO_LIST                                        # every query's five best docs
    lod[-70:] = NO_LIST                                        # and the table's last rows
    sc, ti, bi = tiny_scorer(ss_ctx, 1000)
    try:
        sc.set_doc_vectors(vec)
        sc.set_vector_lists(cent, lod)
        for n_probe in (1, 7):
            got = check_probed(sc, qvec, vec, cent, lod, 100, n_probe, tag=n_probe)
            assert not set(got[0]["doc"].ravel().tolist()) & set(np.flatnonzero(lod == NO_LIST).tolist())
        all_out = np.full(1000, NO_LIST, np.uint32)
        sc.set_vector_lists(cent, all_out)
        got = check_probed(sc, qvec, vec, cent, all_out, 10, 7, tag="no doc in a list")
        assert got[1].tolist() == [0] * 17
    finally:
        close_all(sc, ti, bi)


def test_masks(seg64):
    rng, vec, cent, qvec = world(59, dim=128)
    lod = vlm.assign(vec, cent)[0]
    first = int(vlm.probes(qvec[:1], cent, 1)[0, 0])
    masks = np.zeros((2, 1000), bool)
    masks[0] = rng.random(1000) < 0.5
    masks[1] = lod != first                                    # empties query 0's first list entirely
    mixed = np.array([1, 0, -1, 0, 1, -1, 0, 0, 1, -1, 1, 0, -1, 0, 1, 1, 0], np.int32)
    sc, ti, bi = tiny_scorer(seg64, 1000)
    try:
        sc.set_doc_vectors(vec)
        sc.set_vector_lists(cent, lod)
        sc.set_doc_masks(engine.pack_doc_masks(masks, 1000))
        got = check_probed(sc, qvec, vec, cent, lod, 10, 1, mixed, masks, tag="mixed")
        assert got[1][0] == 0 and got[0][0].tobytes() == bytes([FILL]) * 80        # nothing left of the probed list: the row is untouched
        for n_probe in (2, 7):
            check_probed(sc, qvec, vec, cent, lod, 100, n_probe, mixed, masks, tag=n_probe)
        for one in (0, 1):
            check_probed(sc, qvec, vec, cent, lod, 1000, 3, np.full(17, one, np.int32), masks, tag=("whole", one))
        # a set built by ss_doc_field_masks, registered as it is
        dates = rng.integers(0, 100, (1, 1000)).astype(np.int64)
        sc.set_doc_fields(dates)
        sc.set_doc_masks(sc.doc_field_masks(engine.pack_doc_ranges([[(0, 90, 99)]])))
        check_probed(sc, qvec, vec, cent, lod, 10, 3, np.zeros(17, np.int32), (dates[0] >= 90)[None, :], tag="field mask")
    finally:
        close_all(sc, ti, bi)


# ---- limits and value edges -------------------------------------------------------------------------------------------------------

def test_limits(ss_ctx):
    rng, vec, cent, qvec = world(61, n_docs=3000, n_lists=1500, n_q=5)
    lod = vlm.assign(vec, cent)[0]
    sc, ti, bi = tiny_scorer(ss_ctx, 3000)
    try:
        sc.set_doc_vectors(vec)
        sc.set_vector_lists(cent, lod)
        got = check_probed(sc, qvec, vec, cent, lod, 1024, 1024, tag="k = n_probe = 1024")
        assert (got[1] == 1024).all()
        check_probed(sc, qvec, vec, cent, lod, 1, 1, tag="k = n_probe = 1")
    finally:
        close_all(sc, ti, bi)


@pytest.mark.parametrize("dim", [64, 1024])
def test_value_edges(ss_ctx, dim):
    n_docs = 130
    vec = np.full((n_docs, dim), -128, np.int8)
    half = np.where(np.arange(dim) % 2 == 0, 127, -127).astype(np.int8)
    vec[100:] = half
    qvec = np.stack([np.full(dim, -128, np.int8), np.full(dim, 127, np.int8), half])
    cent = np.stack([np.full(dim, -128, np.int8), half, np.full(dim, 127, np.int8)])
    assert vm.scores(qvec, cent)[0, 0] == dim * 16384
    lod = (np.arange(n_docs) % 3).astype(np.uint32)
    sc, ti, bi = tiny_scorer(ss_ctx, n_docs)
    try:
        sc.set_doc_vectors(vec)
        sc.set_vector_lists(cent, lod)
        for n_probe in (1, 2, 3):
            for k in (1, 50, 130):
                check_probed(sc, qvec, vec, cent, lod, k, n_probe, tag=(dim, n_probe, k))
        want = vlm.assign(vec, cent)
        got = sc.assign_vector_lists(cent, out=(filled(n_docs, np.uint32), filled(n_docs, np.int32)))
        assert as_bytes(got) == as_bytes(want)
    finally:
        close_all(sc, ti, bi)


# ---- the host's query batches, device buffers ---------------------------------------------------------------------------------------

def test_query_batches_give_the_same_bytes(seg64):
    rng, vec, cent, qvec = world(67, n_q=130)
    lod = vlm.assign(vec, cent)[0]
    masks = rng.random((1, 1000)) < 0.5
    mid = (np.arange(130) % 2 - 1).astype(np.int32)
    sc, ti, bi = tiny_scorer(seg64, 1000)
    try:
        sc.set_doc_vectors(vec)
        sc.set_vector_lists(cent, lod)
        sc.set_doc_masks(engine.pack_doc_masks(masks, 1000))
        whole = as_bytes(check_probed(sc, qvec, vec, cent, lod, 10, 3, mid, masks, tag="one batch"))
        for batch in (7, 64, 129):
            seg64.set_option("vec.list_batch_q", batch)
            assert as_bytes(check_probed(sc, qvec, vec, cent, lod, 10, 3, mid, masks, tag=batch)) == whole
    finally:
        close_all(sc, ti, bi)


def test_device_buffers(ss_ctx):
    import torch
    rng, vec, cent, qvec = world(71, dim=128)
    lod = vlm.assign(vec, cent)[0]
    dev = lambda a: torch.from_numpy(a.view(np.uint8) if a.dtype.fields or a.dtype == np.uint32 else a).cuda()      # noqa: E731
    sc, ti, bi = tiny_scorer(ss_ctx, 1000)
    try:
        sc.set_doc_vectors(torch.from_numpy(vec).cuda())
        sc.set_vector_lists(torch.from_numpy(cent).cuda(), dev(lod).view(torch.int32))
        k, n_probe = 10, 3
        want = vlm.topk_probed(qvec, vec, cent, lod, k, n_probe, filled((17, k), engine.VEC_HIT_DTYPE), filled(17, np.int32))
        d_out = (dev(filled((17, k), engine.VEC_HIT_DTYPE)), dev(filled(17, np.int32)), dev(filled((17, n_probe), np.uint32)))
        sc.vector_topk_probed(torch.from_numpy(qvec).cuda(), k, n_probe, out=d_out)
        assert [t.cpu().numpy().tobytes() for t in d_out] == as_bytes(want)
        d_out = (dev(filled((17, k), engine.VEC_HIT_DTYPE)), dev(filled(17, np.int32)))
        sc.vector_topk_probed(torch.from_numpy(qvec).cuda(), k, n_probe, out=d_out)
        assert [t.cpu().numpy().tobytes() for t in d_out] == as_bytes(want[:2])
        lists, scores = sc.assign_vector_lists(torch.from_numpy(cent).cuda(), device_out=True)
        w_lists, w_scores = vlm.assign(vec, cent)
        assert lists.cpu().numpy().tobytes() == w_lists.tobytes() and scores.cpu().numpy().tobytes() == w_scores.tobytes()
    finally:
        close_all(sc, ti, bi)


# ---- assign and train -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_lists", [1, 7, 300])
def test_assign(seg64, n_lists):
    rng, vec, cent, _ = world(73 + n_lists, n_lists=n_lists, lo=-3, hi=4)
    if n_lists > 1:
        cent[n_lists - 1] = cent[0]                            # equal centroids: the lower list
    want = vlm.assign(vec, cent)
    assert n_lists == 1 or not (want[0] == n_lists - 1).any()
    sc, ti, bi = tiny_scorer(seg64, 1000)
    try:
        sc.set_doc_vectors(vec)
        rows = []
        for batch in (None, 300, 64):                          # 1000 docs cross several batches
            seg64.set_option("vec.assign_batch", batch)
            got = sc.assign_vector_lists(cent, out=(filled(1000, np.uint32), filled(1000, np.int32)))
            assert got[0].tolist() == want[0].tolist(), batch
            rows.append(as_bytes(got))
        assert rows == [as_bytes(want)] * 3
        only = sc.assign_vector_lists(cent, out=(filled(1000, np.uint32), None))
        assert only[0].tobytes() == want[0].tobytes() and only[1] is None
    finally:
        close_all(sc, ti, bi)


def test_train_equals_the_model(ss_ctx):
    rng = np.random.default_rng(79)
    centres = rng.integers(-100, 101, (7, 64))
    vec = np.clip(centres[rng.integers(0, 7, 1000)] + rng.integers(-20, 21, (1000, 64)), -128, 127).astype(np.int8)
    want = vlm.train(vec, 7, 3, 11)
    sc, ti, bi = tiny_scorer(ss_ctx, 1000)
    try:
        sc.set_doc_vectors(vec)
        got = engine.train_vector_lists(sc, vec, 7, iters=3, seed=11)
        assert got[0].dtype == np.int8 and got[1].dtype == np.uint32
        assert as_bytes(got) == as_bytes(want)
        sc.set_vector_lists(*got)
        check_probed(sc, vec[:17].copy(), vec, got[0], got[1], 10, 2, tag="trained lists")
    finally:
        close_all(sc, ti, bi)


# ---- errors and lifecycle ---------------------------------------------------------------------------------------------------------

def test_errors_and_lifecycle(ss_ctx):
    n_docs, dim, n_q, k = 200, 64, 4, 5
    rng, vec, cent, qvec = world(83, n_docs=n_docs, n_q=n_q)
    lod = vlm.assign(vec, cent)[0]
    lib = ss_ctx.lib
    ptr = lambda a: None if a is None else a.ctypes.data        # noqa: E731
    sc, ti, bi = tiny_scorer(ss_ctx, n_docs)
    try:
        o_t, o_n, o_p = filled((n_q, k), engine.VEC_HIT_DTYPE), filled(n_q, np.int32), filled((n_q, 3), np.uint32)
        o_l, o_s = filled(n_docs, np.uint32), filled(n_docs, np.int32)
        outs = (o_t, o_n, o_p, o_l, o_s)
        clean = as_bytes(outs)
        probed = lambda nq=n_q, q=qvec, m=None, kk=k, np_=3, h=o_t, n=o_n, p=o_p: lib.ss_vector_topk_probed(   # noqa: E731
            sc.h, nq, ptr(q), ptr(m), kk, np_, ptr(h), ptr(n), ptr(p))
        assign = lambda nl=7, c=cent, lo=o_l, so=o_s: lib.ss_vector_assign_lists(sc.h, nl, ptr(c), ptr(lo), ptr(so))   # noqa: E731
        set_lists = lambda nl=7, c=cent, lo=lod: lib.ss_scorer_set_vector_lists(sc.h, nl, ptr(c), ptr(lo))              # noqa: E731
        # no vector table: nothing works, clearing is fine
        assert probed() == ERR_STATE and assign() == ERR_STATE and set_lists() == ERR_STATE and set_lists(nl=0) == 0
        assert as_bytes(outs) == clean
        sc.set_doc_vectors(vec)
        assert probed() == ERR_STATE and as_bytes(outs) == clean                    # a table, no lists
        with pytest.raises(SpaghettiError) as ei:
            sc.vector_topk_probed(qvec, k, 3)
        assert ei.value.code == ERR_STATE
        sc.set_vector_lists(cent, lod)
        sc.set_doc_masks(engine.pack_doc_masks(np.ones((2, n_docs), bool), n_docs))
        want = as_bytes(vlm.topk_probed(qvec, vec, cent, lod, k, 3, filled((n_q, k), engine.VEC_HIT_DTYPE), filled(n_q, np.int32))[:2])
        for rc, call in ((ERR_INVALID, lambda: lib.ss_vector_topk_probed(None, n_q, ptr(qvec), None, k, 3, ptr(o_t), ptr(o_n), None)),
                         (ERR_INVALID, lambda: probed(nq=-1)), (ERR_INVALID, lambda: probed(q=None)), (ERR_INVALID, lambda: probed(h=None)),
                         (ERR_INVALID, lambda: probed(n=None)), (ERR_INVALID, lambda: probed(kk=0)), (ERR_UNSUPPORTED, lambda: probed(kk=1025)),
                         (ERR_INVALID, lambda: probed(np_=0)), (ERR_INVALID, lambda: probed(np_=-4)), (ERR_UNSUPPORTED, lambda: probed(np_=1025)),
                         (ERR_INVALID, lambda: probed(m=np.array([0, -2, 0, 0], np.int32))),
                         (ERR_INVALID, lambda: probed(m=np.array([0, 1, 2, 0], np.int32))),
                         (ERR_INVALID, lambda: lib.ss_vector_assign_lists(None, 7, ptr(cent), ptr(o_l), ptr(o_s))),
                         (ERR_INVALID, lambda: assign(nl=0)), (ERR_INVALID, lambda: assign(nl=65537)), (ERR_INVALID, lambda: assign(c=None)),
                         (ERR_INVALID, lambda: assign(lo=None)),
                         (ERR_INVALID, lambda: lib.ss_scorer_set_vector_lists(None, 7, ptr(cent), ptr(lod))),
                         (ERR_INVALID, lambda: set_lists(nl=-1)), (ERR_INVALID, lambda: set_lists(nl=65537)), (ERR_INVALID, lambda: set_lists(lo=None))):
            assert call() == rc
            assert as_bytes(outs) == clean
        assert probed(nq=0) == 0 and as_bytes(outs) == clean
        # a bad entry of list_of_doc keeps the old lists
        bad = lod.copy()
        bad[137] = 7
        assert set_lists(lo=bad) == ERR_INVALID
        bad[137] = 0xFFFFFFFE
        assert set_lists(lo=bad) == ERR_INVALID
        assert probed(p=None) == 0 and as_bytes((o_t, o_n)) == want                 # probes_out is optional; the old lists answer
        # other lists replace them
        lod2 = ((lod + 1) % 7).astype(np.uint32)
        sc.set_vector_lists(cent, lod2)
        check_probed(sc, qvec, vec, cent, lod2, k, 3, tag="replaced")
        # ss_scorer_set_doc_vectors drops the lists, replacing or clearing; the exact search is what it was
        exact = as_bytes(sc.vector_topk(qvec, k))
        sc.set_doc_vectors(vec)
        assert as_bytes(sc.vector_topk(qvec, k)) == exact
        o_t[:], o_n[:] = filled(o_t.shape, o_t.dtype), filled(n_q, np.int32)
        assert probed() == ERR_STATE and as_bytes(outs) == clean
        sc.set_vector_lists(cent, lod)
        sc.set_vector_lists(None, None)
        assert probed() == ERR_STATE
        sc.set_vector_lists(cent, lod)
        sc.set_doc_vectors(None)
        assert probed() == ERR_STATE and assign() == ERR_STATE and as_bytes(outs) == clean
    finally:
        close_all(sc, ti, bi)
