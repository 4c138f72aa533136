"""GPU parity: ss_maxsim_topk vs the loops of tests/maxsim_topk_model.py.  Scores are exact integers and ties go to the lower doc, so every
comparison is equality of bytes: tobytes() on whole output arrays that start from 0xA5 bytes, so an entry the call must not write is
checked with the ones it must.  The shapes are the smallest at which k_maxsim_topk takes another path: tile and group seams, query
blocks, chunk seams, shared docs, in-loop compaction."""
import numpy as np
import pytest

from spaghettisearch_amd import SpaghettiError, engine
from tests import maxsim_model as mm
from tests import maxsim_topk_model as tm
from tests.test_gpu_collapse import FILL, filled
from tests.test_gpu_score import close_all
from tests.test_gpu_vector import tiny_scorer
from tests.test_maxsim_topk_cpu import INC, LDS, block_model

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE, ERR_UNSUPPORTED = 1, 6, 7
VEC = engine.VEC_HIT_DTYPE
OPTIONS = ("maxsim.chunk_tokens", "maxsim.wide_tokens")


def ptr_of(counts, dtype):
    p = np.zeros(len(counts) + 1, dtype)
    p[1:] = np.cumsum(counts)
    return p


def outs(n_q, k):
    return filled((n_q, k), VEC), filled(n_q, np.int32)


class World:
    def __init__(self, ss_ctx, tok_ptr, tok, masks=None):
        self.ctx, self.tok_ptr, self.tok, self.masks = ss_ctx, tok_ptr, tok, masks
        self.sc, self.ti, self.bi = tiny_scorer(ss_ctx, len(tok_ptr) - 1)
        self.sc.set_doc_tokens(tok_ptr, tok)
        if masks is not None:
            self.sc.set_doc_masks(engine.pack_doc_masks(masks, len(tok_ptr) - 1))
        self.want = {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for name in OPTIONS:
            self.ctx.set_option(name, None)
        close_all(self.sc, self.ti, self.bi)

    def check(self, qt_ptr, qtok, k, mask_id=None, tag=None, key=None):
        """the call on host arrays against the model, byte for byte -> (hits, n_hits); key: the model's answer is kept under it"""
        n_q = len(qt_ptr) - 1
        if key is None or key not in self.want:
            want = tm.topk(qt_ptr, qtok, self.tok_ptr, self.tok, k, *outs(n_q, k), mask_id=mask_id, masks=self.masks)
            if key is not None:
                self.want[key] = want
        else:
            want = self.want[key]
        got = self.sc.maxsim_topk(qt_ptr, qtok, k, mask_id=None if mask_id is None else np.asarray(mask_id, np.int32), out=outs(n_q, k))
        assert got[1].tolist() == want[1].tolist(), tag
        for q in range(n_q):
            assert got[0][q, :int(want[1][q])].tolist() == want[0][q, :int(want[1][q])].tolist(), (tag, q)
        assert got[0].tobytes() == want[0].tobytes(), tag
        return got


def table(rng, t_d, dim, lo=-128, hi=128):
    tok_ptr = ptr_of(t_d, np.uint64)
    return tok_ptr, rng.integers(lo, hi, (int(tok_ptr[-1]), dim)).astype(np.int8)


# ---- 1: the known answer --------------------------------------------------------------------------------------------------------------

def test_known_answer(ss_ctx):
    tok_ptr, tok, qt_ptr, qtok = mm.known_world()
    with World(ss_ctx, tok_ptr, tok) as w:
        hits, n = w.check(qt_ptr, qtok, 4)
        assert n.tolist() == [3] and hits[0, :3].tolist() == [(0, 16), (1, 12), (3, -11)]
        hits, n = w.check(qt_ptr, qtok, 1)
        assert n.tolist() == [1] and hits[0].tolist() == [(0, 16)]


# ---- 2: tile seams with every product negative ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [64, 192])
def test_tile_seams_negative_products(ss_ctx, dim):
    """a padded token row counted as 0, or a tile the doc does not have, would beat every real (negative) product"""
    rng = np.random.default_rng(41)
    t_d = [1, 15, 16, 17, 47, 48, 49, 63, 64, 65, 127, 128, 129]
    tok_ptr, tok = table(rng, t_d, dim, 1, 6)
    qt_ptr = ptr_of([1, 5, 17, 33], np.uint32)
    qtok = rng.integers(-5, 0, (int(qt_ptr[-1]), dim)).astype(np.int8)
    with World(ss_ctx, tok_ptr, tok) as w:
        hits, n = w.check(qt_ptr, qtok, len(t_d))
        assert n.tolist() == [len(t_d)] * 4 and (hits["score"] < 0).all()
        w.check(qt_ptr, qtok, 3)


# ---- 3: query token counts --------------------------------------------------------------------------------------------------------------

def test_query_token_counts(ss_ctx):
    rng = np.random.default_rng(43)
    t_d = rng.integers(0, 41, 150)
    t_d[:3] = 0
    tok_ptr, tok = table(rng, t_d, 64, -9, 3)                               # mostly negative products: a slot past m_q must not count as 0
    counts = [0, 1, 15, 16, 17, 32, 33, 63, 64]
    with World(ss_ctx, tok_ptr, tok) as w:
        for m in counts:
            qtok = rng.integers(-3, 10, (m, 64)).astype(np.int8)
            hits, n = w.check(ptr_of([m], np.uint32), qtok if m else None, 20, tag=m)
            if m == 0:                                                      # the first k docs that have tokens, score 0
                first = [d for d in range(150) if t_d[d]][:20]
                assert hits[0].tolist() == [(d, 0) for d in first]
        qt_ptr = ptr_of(counts, np.uint32)
        w.check(qt_ptr, rng.integers(-3, 10, (int(qt_ptr[-1]), 64)).astype(np.int8), 20, tag="mixed")


# ---- 4: several query blocks, a mask per query ------------------------------------------------------------------------------------------

def test_query_blocks_and_masks(ss_ctx):
    rng = np.random.default_rng(47)
    n_docs, dim, k = 205, 64, 12
    t_d = rng.integers(0, 6, n_docs)
    t_d[0], t_d[-1] = 2, 3
    tok_ptr, tok = table(rng, t_d, dim, -20, 21)
    assert block_model(dim, 1, k, 1000, LDS)[1] == 16
    n_q = 2 * 16 + 3                                                        # the last block is partial
    masks = np.zeros((6, n_docs), bool)                                     # 0: all-zero
    masks[1] = t_d == 0                                                     # only token-less docs
    masks[2] = rng.random(n_docs) < 0.3
    masks[3, 0] = True                                                      # single docs: the first and the last
    masks[4, n_docs - 1] = True
    masks[5] = rng.random(n_docs) < 0.05
    masks[5, 64:128] = False                                                # a whole group of 64 docs masked out
    qt_ptr = ptr_of(rng.integers(0, 9, n_q), np.uint32)
    qtok = rng.integers(-20, 21, (int(qt_ptr[-1]), dim)).astype(np.int8)
    mask_id = np.array([(-1, 0, 1, 2, 3, 4, 5)[q % 7] for q in range(n_q)], np.int32)
    with World(ss_ctx, tok_ptr, tok, masks) as w:
        words = engine.pack_doc_masks(masks, n_docs).copy()
        words.reshape(6, -1)[:, -1] |= np.uint32(0xFFFFFFFF) << np.uint32(n_docs % 32)     # bits set past n_docs
        w.sc.set_doc_masks(words)
        hits, n = w.check(qt_ptr, qtok, k, mask_id, tag="mixed")
        assert all(n[q] == 0 for q in range(n_q) if mask_id[q] in (0, 1))
        assert all(n[q] == 1 and hits["doc"][q, 0] == (0 if mask_id[q] == 3 else n_docs - 1) for q in range(n_q) if mask_id[q] in (3, 4))
        for one in (0, 1, 4):                                               # a block in which no query may take a doc
            w.check(qt_ptr[:20], qtok, k, np.full(19, one, np.int32), tag=one)
        w.check(qt_ptr, qtok, n_docs + 5, mask_id, tag="every candidate")
        for n in (7, 3, 2):                                                 # blocks of 8, 4 and 2 queries: the kernel's other product paths
            w.check(qt_ptr[:n + 1], qtok, k, mask_id[:n], tag=("block", n))


# ---- 5: forced small chunks -------------------------------------------------------------------------------------------------------------

def test_chunk_seams(ss_ctx):
    rng = np.random.default_rng(53)
    t_d = [0, 0, 64, 0, 30, 34, 0, 0, 3, 61] + rng.integers(1, 6, 40).tolist() + [300] + rng.integers(1, 6, 40).tolist() + [0, 0, 0]
    tok_ptr, tok = table(rng, t_d, 64, -30, 31)
    assert int(tok_ptr[3]) == 64 and int(tok_ptr[6]) == 128 and int(tok_ptr[10]) == 192       # docs ending exactly on a chunk end
    qt_ptr = ptr_of([3, 0, 20], np.uint32)
    qtok = rng.integers(-30, 31, (23, 64)).astype(np.int8)
    with World(ss_ctx, tok_ptr, tok) as w:
        for k in (5, len(t_d)):
            rows = []
            for chunk in (64, 1000, None):
                ss_ctx.set_option("maxsim.chunk_tokens", chunk)
                rows.append(w.check(qt_ptr, qtok, k, tag=(k, chunk), key=k))
            assert len({r[0].tobytes() + r[1].tobytes() for r in rows}) == 1
    # one doc, and a table whose only tokens are one long doc's: every chunk but the first is empty
    for t_d in ([7], [0, 200, 0]):
        tok_ptr, tok = table(rng, t_d, 64, -30, 31)
        with World(ss_ctx, tok_ptr, tok) as w:
            for chunk in (64, None):
                ss_ctx.set_option("maxsim.chunk_tokens", chunk)
                hits, n = w.check(qt_ptr, qtok, 3, tag=(t_d, chunk), key=0)
                assert n.tolist() == [1, 1, 1]
    # a table without a token: no candidate, nothing written but the counts
    with World(ss_ctx, np.zeros(6, np.uint64), np.zeros((0, 64), np.int8)) as w:
        hits, n = w.check(qt_ptr, qtok, 3)
        assert n.tolist() == [0, 0, 0]


# ---- 6: docs the four waves share -------------------------------------------------------------------------------------------------------

def test_wide_docs(ss_ctx):
    rng = np.random.default_rng(59)
    t_d = rng.integers(0, 6, 30).tolist() + [2500] + rng.integers(1, 20, 30).tolist()
    tok_ptr, tok = table(rng, t_d, 64, -128, 128)
    qt_ptr = ptr_of([4, 17, 0, 40], np.uint32)
    qtok = rng.integers(-128, 128, (61, 64)).astype(np.int8)
    with World(ss_ctx, tok_ptr, tok) as w:
        rows = []
        for wide in (1, None, 2 ** 30):
            ss_ctx.set_option("maxsim.wide_tokens", wide)
            rows.append(w.check(qt_ptr, qtok, 10, tag=wide, key=0))
        assert len({r[0].tobytes() + r[1].tobytes() for r in rows}) == 1
        assert 30 in rows[0][0]["doc"][0].tolist()                          # (the long doc has the best token for most query tokens)


# ---- 7: selection -----------------------------------------------------------------------------------------------------------------------

def ramp(n_docs, dim):
    """one token per doc; under the query (100, 1) doc d scores d"""
    tok = np.zeros((n_docs, dim), np.int8)
    tok[:, 0], tok[:, 1] = np.arange(n_docs) // 100, np.arange(n_docs) % 100
    return np.arange(n_docs + 1, dtype=np.uint64), tok


ONE_CHUNK = 2 ** 30                     # "maxsim.chunk_tokens": the whole table in one chunk, so one workgroup's lists take every doc


def test_selection(ss_ctx):
    """Three queries make one block of four; at k = 100 a list holds 356 keys and is cut when it passes 292.  The default plan and the
    forced 64 tokens give chunks of at most 256 and 64 one-token docs, which never get there: only under ONE_CHUNK do the lists overflow
    and vec_compact, the flags and the threshold run inside the loop (about every third group for the rising scores, once for the
    falling and the equal ones, whose later docs the threshold then rejects).  The bytes must not depend on which of them happened."""
    n_docs, dim = 3000, 64
    tok_ptr, tok = ramp(n_docs, dim)
    qtok = np.zeros((3, dim), np.int8)
    qtok[0, :2], qtok[1, :2] = (100, 1), (-100, -1)                         # rising, falling, and all scores equal
    qt_ptr = ptr_of([1, 1, 1], np.uint32)
    assert block_model(dim, 1, 100, 3, LDS)[1:3] == (4, 356) and block_model(dim, 1, 1024, 3, LDS)[1:3] == (4, 2048)
    with World(ss_ctx, tok_ptr, tok) as w:
        for k in (100, 1024, 1):                                            # k = 1024: the lists of 2048 keys are cut in the loop past 1984
            rows = []
            for chunk in (ONE_CHUNK, None, 64):                             # ties by doc ascending, also across chunk boundaries
                ss_ctx.set_option("maxsim.chunk_tokens", chunk)
                hits, n = w.check(qt_ptr, qtok, k, tag=(k, chunk), key=k)
                assert hits[0].tolist() == [(d, d) for d in range(2999, 2999 - k, -1)]
                assert hits[1].tolist() == [(d, -d) for d in range(k)] and hits[2].tolist() == [(d, 0) for d in range(k)]
                rows.append(hits.tobytes() + n.tobytes())
            assert len(set(rows)) == 1
    tok_ptr, tok = ramp(1500, dim)
    with World(ss_ctx, tok_ptr, tok) as w:
        for chunk in (ONE_CHUNK, None):                                     # k = SS_MAX_TOPK with 1500 candidates: in one chunk the lists are cut at its end
            ss_ctx.set_option("maxsim.chunk_tokens", chunk)
            hits, n = w.check(qt_ptr, qtok, 1024, tag=chunk, key=1024)
            assert n.tolist() == [1024] * 3
    with World(ss_ctx, tok_ptr[:51], tok[:50]) as w:
        hits, n = w.check(qt_ptr, qtok, 100)                                # k larger than the candidates
        assert n.tolist() == [50] * 3


def test_selection_tight_lists(ss_ctx):
    """the k at which the plan's lists are as short as they get: k + 64 keys and a handful more; every chunk longer than that cuts them in
    the loop, one chunk of 2000 docs about every group"""
    dim, qt = 128, 4
    slack, k = min((block_model(dim, qt, k, 16, LDS)[2] - (k + INC), k) for k in range(1, 400) if block_model(dim, qt, k, 16, LDS)[1] == 16)
    assert slack < 8
    tok_ptr, tok = ramp(2000, dim)
    qtok = np.zeros((16 * 64, dim), np.int8)
    qtok[::64, :2] = (100, 1)                                               # the first token of every query ranks by doc id, the others score 0
    qtok[64, :2] = (-100, -1)
    with World(ss_ctx, tok_ptr, tok) as w:
        for chunk in (ONE_CHUNK, None):
            ss_ctx.set_option("maxsim.chunk_tokens", chunk)
            hits, n = w.check(ptr_of([64] * 16, np.uint32), qtok, k, tag=chunk, key=0)
            assert hits[0].tolist() == [(d, d) for d in range(1999, 1999 - k, -1)] and hits[1].tolist() == [(d, -d) for d in range(k)]


# ---- 8: extremes ------------------------------------------------------------------------------------------------------------------------

def test_extremes(ss_ctx):
    tok_ptr = ptr_of([3, 0, 1], np.uint64)
    tok = np.full((4, 1024), -128, np.int8)
    with World(ss_ctx, tok_ptr, tok) as w:
        hits, n = w.check(ptr_of([64], np.uint32), np.full((64, 1024), -128, np.int8), 3)
        assert n.tolist() == [2] and hits[0, :2].tolist() == [(0, 2 ** 30), (2, 2 ** 30)]
        hits, n = w.check(ptr_of([64], np.uint32), np.full((64, 1024), 127, np.int8), 3)
        assert hits[0, :2].tolist() == [(0, -64 * 1024 * 127 * 128), (2, -64 * 1024 * 127 * 128)]


# ---- 9: one token per doc and per query: ss_vector_topk ---------------------------------------------------------------------------------

def test_one_token_tables_are_vector_topk(ss_ctx):
    rng = np.random.default_rng(61)
    n_docs, dim, n_q = 500, 128, 20
    vec = rng.integers(-128, 128, (n_docs, dim)).astype(np.int8)
    vec[100:140] = vec[7]                                                   # ties
    qvec = rng.integers(-128, 128, (n_q, dim)).astype(np.int8)
    masks = rng.random((3, n_docs)) < 0.3
    masks[2] = False
    with World(ss_ctx, np.arange(n_docs + 1, dtype=np.uint64), vec, masks) as w:
        w.sc.set_doc_vectors(vec)
        for mask_id in (None, np.array([(-1, 0, 1, 2)[q % 4] for q in range(n_q)], np.int32)):
            for k in (10, 600):
                a = w.sc.vector_topk(qvec, k, mask_id=mask_id, out=outs(n_q, k))
                b = w.sc.maxsim_topk(np.arange(n_q + 1, dtype=np.uint32), qvec, k, mask_id=mask_id, out=outs(n_q, k))
                assert a[1].tobytes() == b[1].tobytes() and a[0].tobytes() == b[0].tobytes(), (k, mask_id is None)


# ---- 10: against ss_hit_maxsim_scores over every doc ------------------------------------------------------------------------------------

def test_rows_are_the_window_scores_sorted(ss_ctx):
    rng = np.random.default_rng(67)
    n_docs, dim, n_q, k = 2000, 128, 40, 50
    tok_ptr, tok = table(rng, rng.integers(0, 41, n_docs), dim)
    qt_ptr = ptr_of(rng.integers(0, 33, n_q), np.uint32)
    qtok = rng.integers(-128, 128, (int(qt_ptr[-1]), dim)).astype(np.int8)
    with World(ss_ctx, tok_ptr, tok) as w:
        sc = np.zeros((n_q, n_docs), np.int64)
        for d0 in range(0, n_docs, 1000):
            hits = np.zeros((n_q, 1000), engine.HIT_DTYPE)
            hits["doc"] = np.arange(d0, d0 + 1000)
            sc[:, d0:d0 + 1000] = w.sc.hit_maxsim_scores(qt_ptr, qtok, hits, np.full(n_q, 1000, np.int32))
        want = outs(n_q, k)
        for q in range(n_q):
            rows = sorted(((d, int(sc[q, d])) for d in range(n_docs) if sc[q, d] != mm.NO_SCORE), key=lambda r: (-r[1], r[0]))[:k]
            want[1][q] = len(rows)
            want[0][q, :len(rows)] = np.array(rows, VEC)
        got = w.sc.maxsim_topk(qt_ptr, qtok, k, out=outs(n_q, k))
        assert got[1].tolist() == want[1].tolist() and got[0].tobytes() == want[0].tobytes()
        # ... and two queries of it against the loops
        w.check(qt_ptr[:3], qtok, k)


# ---- 11: memory kinds, refusals, lifecycle ----------------------------------------------------------------------------------------------

def test_memory_kinds(ss_ctx):
    import torch
    rng = np.random.default_rng(71)
    n_docs, dim, k = 300, 64, 9
    tok_ptr, tok = table(rng, rng.integers(0, 8, n_docs), dim, -20, 21)
    qt_ptr = ptr_of([2, 0, 5, 17], np.uint32)
    qtok = rng.integers(-20, 21, (24, dim)).astype(np.int8)
    masks = rng.random((2, n_docs)) < 0.2
    mask_id = np.array([0, -1, 1, -1], np.int32)
    dev = lambda a: torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).cuda()      # noqa: E731
    with World(ss_ctx, tok_ptr, tok, masks) as w:
        want = w.check(qt_ptr, qtok, k, mask_id)
        d_q = torch.from_numpy(qtok).cuda()
        odd = torch.zeros(qtok.size + 1, dtype=torch.int8, device="cuda")
        odd[1:] = torch.from_numpy(qtok.reshape(-1)).cuda()
        d_q_odd = odd[1:].view(len(qtok), -1)                               # query tokens at an odd address
        assert d_q_odd.data_ptr() % 16 == 1
        d_ptr, d_mid = torch.from_numpy(qt_ptr.view(np.int32)).cuda(), torch.from_numpy(mask_id).cuda()
        for q_arg in (qtok, d_q, d_q_odd):
            for p_arg, m_arg in ((qt_ptr, mask_id), (d_ptr, d_mid), (qt_ptr, d_mid)):
                for o in (outs(4, k), tuple(dev(a) for a in outs(4, k)), (dev(outs(4, k)[0]), outs(4, k)[1]), (outs(4, k)[0], dev(outs(4, k)[1]))):
                    got = w.sc.maxsim_topk(p_arg, q_arg, k, mask_id=m_arg, out=o)
                    got = [t.cpu().numpy() if hasattr(t, "cpu") else t for t in got]
                    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        # all device: the rows go on to a second call on the same stream (what ss_score_docs takes is what ss_hit_maxsim_scores reads)
        d_o = tuple(dev(a) for a in outs(4, k))
        w.sc.maxsim_topk(qt_ptr, d_q, k, mask_id=d_mid, out=d_o)
        rows = d_o[0].cpu().numpy().view(VEC).reshape(4, k)
        hits = np.zeros((4, k), engine.HIT_DTYPE)
        hits["doc"] = rows["doc"]
        again = w.sc.hit_maxsim_scores(qt_ptr, qtok, hits, want[1])
        assert all(again[q, :want[1][q]].tolist() == want[0]["score"][q, :want[1][q]].tolist() for q in range(4))


def test_refusals_leave_outputs_untouched(ss_ctx):
    rng = np.random.default_rng(73)
    n_docs, dim = 100, 64
    tok_ptr, tok = table(rng, rng.integers(0, 8, n_docs), dim, -20, 21)
    qt_ptr = ptr_of([2, 5], np.uint32)
    qtok = rng.integers(-20, 21, (70, dim)).astype(np.int8)
    lib, raw = ss_ctx.lib, lambda a: None if a is None else a.ctypes.data       # noqa: E731

    def refused(sc, code, n_q=2, ptr=qt_ptr, q=qtok, mid=None, k=5, no_out=False):
        o = outs(2, max(min(k, 1024), 1))
        rc = lib.ss_maxsim_topk(sc.h, n_q, raw(ptr), raw(q), raw(mid), k, None if no_out else raw(o[0]), raw(o[1]))
        assert rc == code, (rc, code)
        assert o[0].tobytes() == bytes([FILL]) * o[0].nbytes and o[1].tobytes() == bytes([FILL]) * o[1].nbytes

    sc, ti, bi = tiny_scorer(ss_ctx, n_docs)
    try:
        refused(sc, ERR_STATE)                                              # before a table exists
        refused(sc, ERR_STATE, n_q=0)                                       # ... which is asked for before n_q == 0, as in the sibling calls
        sc.set_doc_tokens(tok_ptr, tok)
        sc.set_doc_masks(engine.pack_doc_masks(np.ones((2, n_docs), bool), n_docs))
        refused(sc, ERR_INVALID, n_q=-1)
        refused(sc, ERR_INVALID, k=0)
        refused(sc, ERR_UNSUPPORTED, k=1025)
        refused(sc, ERR_INVALID, no_out=True)
        refused(sc, ERR_INVALID, ptr=None)
        refused(sc, ERR_INVALID, q=None)                                    # the call has query tokens
        refused(sc, ERR_INVALID, ptr=np.array([5, 3, 4], np.uint32))        # a decreasing qt_ptr
        refused(sc, ERR_UNSUPPORTED, ptr=np.array([0, 65, 70], np.uint32))  # 65 query tokens
        refused(sc, ERR_INVALID, mid=np.array([0, 2], np.int32))
        refused(sc, ERR_INVALID, mid=np.array([-2, 0], np.int32))
        refused(sc, 0, n_q=0)                                               # SS_OK, and nothing is done
        o = outs(2, 5)
        assert lib.ss_maxsim_topk(sc.h, 2, raw(np.array([4, 4, 4], np.uint32)), None, None, 5, raw(o[0]), raw(o[1])) == 0   # no query token: qtok may be NULL
        assert o[1].tolist() == [5, 5]
        sc.set_doc_tokens(None, None)
        refused(sc, ERR_STATE)                                              # after the table is cleared
    finally:
        close_all(sc, ti, bi)


def test_table_replaced_between_calls(ss_ctx):
    rng = np.random.default_rng(79)
    n_docs = 150
    qt_ptr = ptr_of([3, 9], np.uint32)
    tok_ptr, tok = table(rng, rng.integers(0, 8, n_docs), 64, -20, 21)
    with World(ss_ctx, tok_ptr, tok) as w:
        first = w.check(qt_ptr, rng.integers(-20, 21, (12, 64)).astype(np.int8), 8)
        w.tok_ptr, w.tok = table(rng, rng.integers(0, 200, n_docs), 128, -20, 21)     # another dim, far more slices
        w.sc.set_doc_tokens(w.tok_ptr, w.tok)
        second = w.check(qt_ptr, rng.integers(-20, 21, (12, 128)).astype(np.int8), 8)
        assert first[0].tobytes() != second[0].tobytes()
        w.tok_ptr, w.tok = np.zeros(n_docs + 1, np.uint64), np.zeros((0, 64), np.int8)    # ... and one without a token
        w.sc.set_doc_tokens(w.tok_ptr, w.tok)
        assert w.check(qt_ptr, rng.integers(-20, 21, (12, 64)).astype(np.int8), 8)[1].tolist() == [0, 0]
