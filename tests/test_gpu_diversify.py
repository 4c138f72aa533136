"""GPU parity: ss_diversify_hits vs the numpy restatement of the header's definition (tests/diversify_model.py).  Similarities and
relevance are exact integers and ties break by window index, so every comparison is equality of bytes: tobytes() on whole output arrays
that start from 0xA5 bytes, so an entry the call must not write is checked with the ones it must."""
import numpy as np
import pytest

from spaghettisearch_amd import SpaghettiError, engine
from tests import diversify_model as dm
from tests.test_gpu_collapse import FILL, as_bytes, filled, random_rows
from tests.test_gpu_score import close_all
from tests.test_gpu_vector import tiny_scorer

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE, ERR_UNSUPPORTED = 1, 6, 7
NO = dm.NO_SCORE
WEIGHTS = [(65536, 65536), (2, 1), (0, 1), (1, 0), (0, 0)]


def outs(n_q, k, info=True):
    return filled((n_q, k), engine.HIT_DTYPE), filled(n_q, np.int32), filled((n_q, k), engine.DIV_INFO_DTYPE) if info else None


def check(sc, qvec, vec, hits, n_hits, w_rel, w_div, first=0, k=None, tag=None):
    """the call on host arrays against the model, byte for byte -> the call's outputs"""
    n_q = hits.shape[0]
    k = hits.shape[1] if k is None else k
    want = dm.diversify(qvec, vec, hits, n_hits, w_rel, w_div, first, k, *outs(n_q, k))
    got = sc.diversify_hits(qvec, hits, n_hits, k, w_rel, w_div, first=first, out=outs(n_q, k))
    assert got[1].tolist() == want[1].tolist(), tag
    for q in range(n_q):
        n = int(want[1][q])
        assert got[0]["doc"][q, :n].tolist() == want[0]["doc"][q, :n].tolist(), (tag, q)
        assert got[2][q, :n].tolist() == want[2][q, :n].tolist(), (tag, q)
    assert as_bytes(got) == as_bytes(want), tag
    return got


def rows_of(rng, docs):
    docs = np.asarray(docs)
    hits = random_rows(rng, docs.shape[0], docs.shape[1], 1)      # random bytes in _pad and the scores: carried through
    hits["doc"] = docs
    return hits


class World:
    def __init__(self, ss_ctx, vec):
        self.vec = vec
        self.sc, self.ti, self.bi = tiny_scorer(ss_ctx, vec.shape[0])
        self.sc.set_doc_vectors(vec)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        close_all(self.sc, self.ti, self.bi)


# ---- the known answer ---------------------------------------------------------------------------------------------------------------

def test_known_answer(ss_ctx):
    vec = np.zeros((4, 64), np.int8)
    vec[:, :2] = [(10, 0), (9, 1), (0, 8), (5, 5)]
    qvec = np.zeros((1, 64), np.int8)
    qvec[0, 0] = 1
    hits = rows_of(np.random.default_rng(1), [[0, 1, 2, 3]])
    n_hits = np.array([4], np.int32)
    with World(ss_ctx, vec) as w:
        got = check(w.sc, qvec, vec, hits, n_hits, 2, 1)
        assert got[0]["doc"][0].tolist() == [0, 2, 3, 1] and got[2][0].tolist() == [(10, NO), (0, 0), (5, 50), (9, 90)]
        assert check(w.sc, qvec, vec, hits, n_hits, 1, 0)[0]["doc"][0].tolist() == [0, 1, 3, 2]
        assert check(w.sc, None, vec, hits, n_hits, 30, 1)[0]["doc"][0].tolist() == [0, 2, 1, 3]


# ---- operand layout -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [64, 192])
def test_operand_layout(ss_ctx, dim):
    """one-hot docs against docs with a distinct weight per position, in one window: sim(one-hot, dense) is one product, so a permuted
    k order on one operand, a row / column swap or an unsummed k step each give wrong penalties"""
    n_hot, n_dense = 2 * dim, 9
    vec = np.zeros((n_hot + n_dense, dim), np.int8)
    d = np.arange(n_hot)
    vec[d, d % dim] = 1 + d % 7
    i = np.arange(dim)
    for x in range(n_dense):
        vec[n_hot + x] = ((i * 37 + x * 11) % 251) - 125
    assert all(len(set(r.tolist())) == 64 for r in vec[n_hot:, :64])
    rng = np.random.default_rng(dim)
    n = 130
    docs = np.stack([rng.permutation(np.concatenate([rng.choice(n_hot, n - n_dense, replace=False), n_hot + np.arange(n_dense)]))
                     for _ in range(3)])
    hits = rows_of(rng, docs)
    n_hits = np.full(3, n, np.int32)
    assert len(np.unique(dm.gram(vec, docs[0]))) > 20           # the similarities are many different products
    with World(ss_ctx, vec) as w:
        for w_rel, w_div in ((0, 1), (1, 1), (3, 2)):
            check(w.sc, None, vec, hits, n_hits, w_rel, w_div, tag=(dim, w_rel, w_div))
        check(w.sc, vec[n_hot:n_hot + 3], vec, hits, n_hits, 1, 1, tag=(dim, "qvec"))


# ---- shapes -------------------------------------------------------------------------------------------------------------------------

SHAPES = [([0], 1, 64, 70), ([1], 1, 192, 70), ([2, 1, 0], 2, 64, 70), ([63, 64, 2], 64, 192, 4099), ([65, 63, 64], 65, 1024, 70),
          ([64], 64, 1024, 4099), ([130, 65, 0], 130, 64, 70), ([130], 130, 192, 4099), ([63], 128, 64, 70), ([2], 129, 64, 4099),
          ([0, 1, 2, 63, 64, 65, 130, 200, 199, 128, 127, 129, 1, 64, 65, 0, 200], 200, 64, 4099),
          ([1024], 1024, 64, 4099), ([1024, 130, 1000], 1024, 192, 70), ([1024], 1024, 1024, 70)]


@pytest.mark.parametrize("n_list,k_in,dim,n_docs", SHAPES)
def test_shapes(ss_ctx, n_list, k_in, dim, n_docs):
    rng = np.random.default_rng(k_in * 7 + dim + n_docs + len(n_list))
    n_q = len(n_list)
    vec = rng.integers(-128, 128, (n_docs, dim)).astype(np.int8)
    qvec = rng.integers(-128, 128, (n_q, dim)).astype(np.int8)
    hits = rows_of(rng, rng.integers(0, n_docs, (n_q, k_in)))             # n_docs = 70: the windows repeat docs
    n_hits = np.array(n_list, np.int32)
    weights = WEIGHTS if k_in < 1024 else [(65536, 65536), (2, 1), (0, 1)]
    with World(ss_ctx, vec) as w:
        for w_rel, w_div in weights:
            for qv in (qvec, None):
                check(w.sc, qv, vec, hits, n_hits, w_rel, w_div, tag=(w_rel, w_div, qv is None))


def test_shape_grid_holds_every_value():
    ns = {n for s in SHAPES for n in s[0]}
    assert {0, 1, 2, 63, 64, 65, 130, 1024} <= ns
    assert {s[2] for s in SHAPES} == {64, 192, 1024} and {len(s[0]) for s in SHAPES} == {1, 3, 17} and {s[3] for s in SHAPES} == {70, 4099}
    assert any(max(s[0]) == s[1] for s in SHAPES) and any(max(s[0]) < s[1] for s in SHAPES)
    assert {s[1] for s in SHAPES} >= {128, 129}                              # both select kernels: a window of up to 128 rows, and above


# ---- tile seams ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,pair", [(130, (63, 64)), (130, (127, 128)), (130, (0, 129)), (65, (0, 64)), (1024, (0, 1023)), (1024, (511, 960))])
def test_tile_seams(ss_ctx, n, pair):
    """orthogonal docs but for one similar pair, which sits on both sides of a tile seam: the later row of the pair is chosen last"""
    dim = 1024 if n > 192 else 192
    vec = np.zeros((n, dim), np.int8)
    vec[np.arange(n), np.arange(n)] = 10
    a, b = pair
    vec[b, a] = 9                                               # sim(a, b) = 90; every other pair 0
    hits = rows_of(np.random.default_rng(n + a), [np.arange(n)])
    n_hits = np.array([n], np.int32)
    with World(ss_ctx, vec) as w:
        got = check(w.sc, None, vec, hits, n_hits, 1, 65536, tag=pair)
        order = got[0]["doc"][0].tolist()
        assert order[-1] == b and order[:-1] == [j for j in range(n) if j != b]
        assert got[2]["sim"][0, -1] == 90 and set(got[2]["sim"][0, 1:-1].tolist()) == {0}
        qvec = np.zeros((1, dim), np.int8)
        qvec[0, a], qvec[0, b] = 2, 3                           # b is the most relevant row, a the next: a pays for b
        got = check(w.sc, qvec, vec, hits, n_hits, 1, 1, tag=pair)
        assert got[0]["doc"][0, 0] == b and got[0]["doc"][0, -1] == a and got[2][0, -1].tolist() == (20, 90)


# ---- value edges --------------------------------------------------------------------------------------------------------------------

def test_value_edges(ss_ctx):
    dim, n_docs = 1024, 12
    half = np.where(np.arange(dim) % 2 == 0, 127, -127).astype(np.int8)
    vec = np.zeros((n_docs, dim), np.int8)
    vec[0:3] = -128                                             # sim = 2^24
    vec[3:5] = 0                                                # zero vectors
    vec[5:7] = half                                             # against all-127 rows the exact sum is 0
    vec[7:9] = 127
    vec[9:11] = -127                                            # against the 127 rows: a negative sim, a bonus
    vec[11] = -128
    qvec = np.stack([np.full(dim, -128, np.int8), np.full(dim, 127, np.int8), half, np.zeros(dim, np.int8)])
    g = dm.gram(vec, np.arange(n_docs))
    assert g[0, 1] == 2 ** 24 and g[5, 7] == 0 and g[7, 9] == -127 * 127 * dim and g[3, 0] == 0
    rng = np.random.default_rng(3)
    docs = np.stack([np.array([0, 1, 2, 11] * 3), np.arange(n_docs), rng.permutation(n_docs), np.array([7, 9, 8, 10, 5, 3] * 2)])
    hits = rows_of(rng, docs)
    n_hits = np.full(4, n_docs, np.int32)
    with World(ss_ctx, vec) as w:
        for w_rel, w_div in WEIGHTS:
            for qv in (qvec, None):
                check(w.sc, qv, vec, hits, n_hits, w_rel, w_div, tag=(w_rel, w_div, qv is None))
        got = check(w.sc, qvec, vec, hits, n_hits, 65536, 65536)
        assert got[2][0, 1].tolist() == (2 ** 24, 2 ** 24)                   # value = 2^40 - 2^40 at the largest weights
        got = check(w.sc, None, vec, hits, n_hits, 0, 1)
        assert got[0]["doc"][3, :2].tolist() == [7, 9]                      # the row with the negative sim follows the first row


@pytest.mark.parametrize("dim", [64, 1024])
def test_all_zero_and_identical_vectors(ss_ctx, dim):
    rng = np.random.default_rng(dim)
    n_docs, n = 140, 130
    docs = np.stack([rng.permutation(n_docs)[:n] for _ in range(2)])
    hits = rows_of(rng, docs)
    n_hits = np.full(2, n, np.int32)
    qvec = rng.integers(-128, 128, (2, dim)).astype(np.int8)
    for vec in (np.zeros((n_docs, dim), np.int8), np.tile(rng.integers(-128, 128, (1, dim)).astype(np.int8), (n_docs, 1))):
        with World(ss_ctx, vec) as w:
            for w_rel, w_div in WEIGHTS:
                for qv in (qvec, None):
                    got = check(w.sc, qv, vec, hits, n_hits, w_rel, w_div)
                    assert got[0].tobytes() == hits.tobytes()               # every value ties at every step: the window order
    # identical vectors but for their length: rel decides, then the index
    vec = np.zeros((n_docs, dim), np.int8)
    vec[:, 0] = rng.integers(1, 4, n_docs)
    qvec[:] = 0
    qvec[:, 0] = 1
    with World(ss_ctx, vec) as w:
        got = check(w.sc, qvec, vec, hits, n_hits, 1, 0)
        for q in range(2):
            assert got[0]["doc"][q].tolist() == [int(docs[q, j]) for j in sorted(range(n), key=lambda j: (-int(vec[docs[q, j], 0]), j))]
        check(w.sc, qvec, vec, hits, n_hits, 3, 1)


# ---- rows and paging ----------------------------------------------------------------------------------------------------------------

def paging_world():
    rng = np.random.default_rng(29)
    n_docs, dim, k_in = 300, 64, 140
    vec = rng.integers(-20, 21, (n_docs, dim)).astype(np.int8)
    qvec = rng.integers(-20, 21, (4, dim)).astype(np.int8)
    docs = rng.integers(0, n_docs, (4, k_in))
    docs[:, 3] = docs[:, 77]                                    # the same doc twice, in two tiles
    docs[:, 4] = docs[:, 5]                                     # ... and side by side
    docs[0, [0, 9, 64, 100, 139]] = [n_docs, 0xFFFFFFFF, n_docs + 1, 0x80000000, n_docs]     # outside rows interleaved
    docs[1, :] = rng.integers(n_docs, 2 ** 32, k_in)            # an all-outside window
    docs[2, 50:] = n_docs                                       # most rows outside
    hits = rows_of(rng, docs)
    n_hits = np.array([k_in, k_in, 131, 67], np.int32)
    return vec, qvec, hits, n_hits


def test_rows_and_paging(ss_ctx):
    vec, qvec, hits, n_hits = paging_world()
    n, n_inside = 140, 135                                      # of window 0
    with World(ss_ctx, vec) as w:
        for qv in (qvec, None):
            for first in (0, n_inside - 1, n_inside, n, n + 1, 3, 49, 50, 66, 67, 130, 131):
                for k in (1, 7, 1024):                          # pages that end inside the chosen rows, cross into the outside rows, start there
                    check(w.sc, qv, vec, hits, n_hits, 3, 2, first=first, k=k, tag=(first, k, qv is None))
        got = check(w.sc, qvec, vec, hits, n_hits, 3, 2, first=n_inside - 2, k=5)
        assert got[2][0].tolist()[2:] == [(NO, NO)] * 3 and got[2][0, 1]["rel"] != NO
        assert got[0]["doc"][0, 2:].tolist() == [300, 0xFFFFFFFF, 301]
        got = check(w.sc, qvec, vec, hits, n_hits, 3, 2)
        assert got[0][1].tobytes() == hits[1].tobytes() and set(got[2][1].tolist()) == {(NO, NO)}      # all outside: the window as it is
        assert sorted(got[0]["doc"][3, :67].tolist()) == sorted(hits["doc"][3, :67].tolist())
        # info_out is optional
        got = w.sc.diversify_hits(qvec, hits, n_hits, 10, 3, 2, first=2, out=outs(4, 10, info=False))
        want = dm.diversify(qvec, vec, hits, n_hits, 3, 2, 2, 10, *outs(4, 10, info=False))
        assert as_bytes(got) == as_bytes(want)


# ---- identities ---------------------------------------------------------------------------------------------------------------------

def test_identities_on_the_device(ss_ctx):
    vec, qvec, hits, n_hits = paging_world()
    vec[:, 4:] = 0                                              # few distinct scores: equal scores inside every window
    n_q, k_in = hits.shape
    with World(ss_ctx, vec) as w:
        scores = w.sc.hit_vector_scores(qvec, hits, n_hits, out=filled((n_q, k_in), np.int32))
        for first, k in ((0, k_in), (5, 10), (130, 20)):
            rr = w.sc.rerank_hits_by_vector(qvec, hits, n_hits, k, first=first, out=(filled((n_q, k), engine.HIT_DTYPE), filled(n_q, np.int32),
                                                                                     filled((n_q, k), np.int32)))
            for w_rel in (1, 65536):
                got = w.sc.diversify_hits(qvec, hits, n_hits, k, w_rel, 0, first=first, out=outs(n_q, k))
                assert as_bytes(got[:2]) == as_bytes(rr[:2])
                for q in range(n_q):
                    assert got[2]["rel"][q, :got[1][q]].tolist() == rr[2][q, :rr[1][q]].tolist()
        # info.rel is the row's entry of hit_vector_scores
        got = w.sc.diversify_hits(qvec, hits, n_hits, k_in, 2, 1, out=outs(n_q, k_in))
        for q in range(n_q):
            n = int(n_hits[q])
            by_row = {hits[q, j].tobytes(): int(scores[q, j]) for j in range(n)}
            assert all(by_row[got[0][q, r].tobytes()] == int(got[2]["rel"][q, r]) for r in range(n))
        # by rank, without diversity: the window with its inside rows first
        got = w.sc.diversify_hits(None, hits, n_hits, k_in, 1, 0, out=outs(n_q, k_in))
        for q in range(n_q):
            n = int(n_hits[q])
            order = sorted(range(n), key=lambda j: (hits["doc"][q, j] >= vec.shape[0], j))
            assert got[0][q, :n].tobytes() == hits[q, order].tobytes()


# ---- groups -------------------------------------------------------------------------------------------------------------------------

def test_groups_give_the_same_bytes(ss_ctx):
    rng = np.random.default_rng(31)
    n_docs, dim, n_q, k_in = 500, 64, 17, 130
    vec = rng.integers(-128, 128, (n_docs, dim)).astype(np.int8)
    qvec = rng.integers(-128, 128, (n_q, dim)).astype(np.int8)
    hits = rows_of(rng, rng.integers(0, n_docs + 20, (n_q, k_in)))
    n_hits = rng.integers(0, k_in + 1, n_q).astype(np.int32)
    n_hits[[0, 8, 9, 16]] = k_in                               # full windows on both sides of every group seam
    qb = 192 * 192 * 4                                          # one query's Gram matrix: pitch 192
    with World(ss_ctx, vec) as w:
        try:
            base = as_bytes(check(w.sc, qvec, vec, hits, n_hits, 2, 1))
            for scratch in (17 * qb, 9 * qb, 2 * qb - 1, qb, qb - 1, 1):          # 1, 2, 17, 17, 17 (too small for one), 17 groups
                ss_ctx.set_option("div.scratch_bytes", scratch)
                assert as_bytes(check(w.sc, qvec, vec, hits, n_hits, 2, 1, tag=scratch)) == base
                check(w.sc, None, vec, hits, n_hits, 1, 1, first=3, k=9, tag=scratch)
        finally:
            ss_ctx.set_option("div.scratch_bytes", None)


# ---- counts and pointer mixes -------------------------------------------------------------------------------------------------------

def test_counts_and_pointer_mixes(ss_ctx):
    import torch
    vec, qvec, hits, n_hits = paging_world()
    n_q, k_in = hits.shape
    dev = lambda a: torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).cuda()      # noqa: E731
    with World(ss_ctx, vec) as w:
        d_hits, d_q = dev(hits), torch.from_numpy(qvec).cuda()
        odd = torch.zeros(qvec.size + 1, dtype=torch.int8, device="cuda")
        odd[1:] = torch.from_numpy(qvec.reshape(-1)).cuda()
        d_q_odd = odd[1:].view(n_q, -1)                          # query vectors at an odd address
        assert d_q_odd.data_ptr() % 16 == 1
        for counts in (n_hits, np.array([-5, k_in + 9, 2, k_in], np.int32)):
            for first, k in ((0, k_in), (4, 9)):
                for qv, dq in ((qvec, d_q), (qvec, d_q_odd), (None, None)):
                    want = dm.diversify(qv, vec, hits, counts, 3, 2, first, k, *outs(n_q, k), clamp=True)
                    d_n = dev(counts)
                    d_out = tuple(dev(a) for a in outs(n_q, k))
                    w.sc.diversify_hits(dq, d_hits, d_n, k, 3, 2, first=first, k_in=k_in, out=d_out)              # all device
                    assert [t.cpu().numpy().tobytes() for t in d_out] == as_bytes(want), (first, k)
                    got = w.sc.diversify_hits(qv, hits, d_n, k, 3, 2, first=first, k_in=k_in, out=outs(n_q, k))   # host rows, device counts
                    assert as_bytes(got) == as_bytes(want), (first, k)
                    h_out = outs(n_q, k)
                    mixed = (dev(h_out[0]), h_out[1], dev(h_out[2]))
                    w.sc.diversify_hits(dq, hits, d_n, k, 3, 2, first=first, k_in=k_in, out=mixed)                # device rows out, host counts out
                    assert [mixed[0].cpu().numpy().tobytes(), mixed[1].tobytes(), mixed[2].cpu().numpy().tobytes()] == as_bytes(want)
        # host counts outside the window are refused, outputs untouched
        for bad in (np.array([-5, 1, 1, 1], np.int32), np.array([1, k_in + 9, 1, 1], np.int32)):
            o = outs(n_q, 5)
            with pytest.raises(SpaghettiError) as ei:
                w.sc.diversify_hits(qvec, hits, bad, 5, 3, 2, out=o)
            assert ei.value.code == ERR_INVALID and as_bytes(o) == as_bytes(outs(n_q, 5))


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
        o_h, o_n, o_i = outs(n_q, k)
        clean = as_bytes((o_h, o_n, o_i))
        call = lambda nq=n_q, q=qvec, ki=k, h=hits, n=n_hits, wr=2, wd=1, first=0, kk=k, oh=o_h, on=o_n, oi=o_i: lib.ss_diversify_hits(   # noqa: E731
            sc.h, nq, ptr(q), ki, ptr(h), ptr(n), wr, wd, first, kk, ptr(oh), ptr(on), ptr(oi))
        assert call() == ERR_STATE and call(q=None) == ERR_STATE                       # no vector table
        assert call(wr=-1) == ERR_INVALID                                              # (the arguments are checked before the state)
        assert as_bytes((o_h, o_n, o_i)) == clean
        sc.set_doc_vectors(vec)
        for rc, bad in ((ERR_INVALID, lambda: lib.ss_diversify_hits(None, n_q, ptr(qvec), k, ptr(hits), ptr(n_hits), 2, 1, 0, k, ptr(o_h), ptr(o_n), ptr(o_i))),
                        (ERR_INVALID, lambda: call(nq=-1)), (ERR_INVALID, lambda: call(ki=0)), (ERR_INVALID, lambda: call(kk=0)),
                        (ERR_INVALID, lambda: call(first=-1)), (ERR_UNSUPPORTED, lambda: call(ki=1025)), (ERR_UNSUPPORTED, lambda: call(kk=1025)),
                        (ERR_INVALID, lambda: call(h=None)), (ERR_INVALID, lambda: call(n=None)), (ERR_INVALID, lambda: call(oh=None)),
                        (ERR_INVALID, lambda: call(on=None)), (ERR_INVALID, lambda: call(n=np.array([k + 1, 0, 0, 0], np.int32))),
                        (ERR_INVALID, lambda: call(n=np.array([0, 0, -1, 0], np.int32))),
                        (ERR_INVALID, lambda: call(wr=-1)), (ERR_INVALID, lambda: call(wd=-1)), (ERR_INVALID, lambda: call(wr=65537)),
                        (ERR_INVALID, lambda: call(wd=65537)), (ERR_INVALID, lambda: call(q=None, wd=2 ** 31 - 1))):
            assert bad() == rc
            assert as_bytes((o_h, o_n, o_i)) == clean
        both = filled((n_q, 2 * k), engine.HIT_DTYPE)
        assert lib.ss_diversify_hits(sc.h, n_q, ptr(qvec), k, ptr(both), ptr(n_hits), 2, 1, 0, k, both.ctypes.data + 40, ptr(o_n), None) == ERR_INVALID
        assert as_bytes((o_h, o_n, o_i)) == clean and both.tobytes() == bytes([FILL]) * both.nbytes
        assert call(nq=0) == 0 and call(nq=0, q=None) == 0 and as_bytes((o_h, o_n, o_i)) == clean
        assert call(oi=None) == 0 and o_i.tobytes() == clean[2]                        # info_out is optional
        assert call(q=None) == 0 and call(wr=0, wd=0) == 0 and call(wr=65536, wd=65536) == 0
        with pytest.raises(SpaghettiError) as ei:
            sc.diversify_hits(qvec, hits, n_hits, k, 70000, 1)
        assert ei.value.code == ERR_INVALID
        with pytest.raises(SpaghettiError):
            ss_ctx.set_option("div.no_such_option", 1)
        sc.set_doc_vectors(None)
        o_h[:], o_n[:], o_i[:] = outs(n_q, k)
        assert call() == ERR_STATE and as_bytes((o_h, o_n, o_i)) == clean
    finally:
        close_all(sc, ti, bi)
