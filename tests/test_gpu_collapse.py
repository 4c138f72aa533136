"""GPU parity: "collapse by group" (ss_scorer_set_doc_groups, ss_collapse_hits, ss_score_topk_collapsed) vs the sequential model
(tests/collapse_model.py).  Every comparison is bit-exact: tobytes() on whole output arrays that start from 0xA5 bytes, so an entry the
call must not write is checked with the ones it must."""
import os

import numpy as np
import pytest

from spaghettisearch_amd import SpaghettiError, engine
from tests import collapse_model as cm
from tests.test_gpu_score import close_all, make_scorer

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE, ERR_UNSUPPORTED = 1, 6, 7
NO = cm.NO_GROUP
UNKNOWN = 0xFFFFFFFF
FILL = 0xA5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "index_300x80.npz")
EDGE_VALUES = [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE]


def filled(shape, dtype):
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return np.frombuffer(bytes([FILL]) * n, dtype=dtype).reshape(shape).copy()


def outputs(n_q, k):
    return filled((n_q, k), engine.HIT_DTYPE), filled(n_q, np.int32), filled((n_q, k), np.uint32), filled(n_q, np.int32)


def as_bytes(out):
    return [None if a is None else np.ascontiguousarray(a).tobytes() for a in out]


def want(hits, n_hits, group, g, first, k, same=True, kept=True, clamp=False):
    o = outputs(hits.shape[0], k)
    o = (o[0], o[1], o[2] if same else None, o[3] if kept else None)
    return cm.collapse(hits, n_hits, group, g, first, k, *o, clamp=clamp)


def check(sc, hits, n_hits, group, g, first, k, tag=None):
    """host arrays in, host arrays out, against the model"""
    got = sc.collapse_hits(hits, n_hits, g, k, first=first, out=outputs(hits.shape[0], k))
    assert as_bytes(got) == as_bytes(want(hits, n_hits, group, g, first, k)), (tag, g, first, k)
    return got


def random_rows(rng, n_q, k_in, doc_hi):
    """rows of random BYTES (NaN, -0.0, anything in _pad and the scores; not sorted by anything) with docs below doc_hi"""
    hits = np.frombuffer(rng.bytes(n_q * k_in * 40), dtype=engine.HIT_DTYPE).reshape(n_q, k_in).copy()
    hits["doc"] = rng.integers(0, doc_hi, (n_q, k_in))
    return hits


@pytest.fixture(scope="module")
def world():
    z = np.load(GOLDEN)
    n_docs = int(z["n_docs"])
    rng = np.random.default_rng(21)
    # a third of the docs on twelve small sites, the edge values among them; a third on one big site; the rest never collapsed
    group = np.full(n_docs, NO, np.uint32)
    pick = rng.random(n_docs)
    group[pick < 0.33] = rng.choice(np.array(EDGE_VALUES + [5, 6, 7, 8, 9, 10, 11], np.uint32), int((pick < 0.33).sum()))
    group[pick > 0.67] = 77
    return {"n_docs": n_docs, "n_terms": len(z["b_ptr"]) - 1, "title": (z["t_ptr"], z["t_doc"], z["t_w"]),
            "body": (z["b_ptr"], z["b_doc"], z["b_w"]), "mt": z["t_mag"], "mb": z["b_mag"], "group": group}


@pytest.fixture()
def scorer(ss_ctx, world):
    sc, ti, bi = make_scorer(ss_ctx, world["n_docs"], world["title"], world["body"], world["mt"], world["mb"])
    sc.set_doc_groups(world["group"])
    yield sc, ti, bi
    close_all(sc, ti, bi)


# the edges of a wave (64), of the one-wave kernel (128), of the four-wave block (256) and of the power-of-two padding
@pytest.mark.parametrize("k_in", [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024])
def test_window_sizes(world, scorer, k_in):
    sc = scorer[0]
    rng = np.random.default_rng(k_in)
    lengths = list(range(k_in + 1)) if k_in <= 65 else [0, 1, k_in - 1, k_in, k_in // 2, k_in // 2 + 1]
    n_hits = np.array(lengths, np.int32)
    hits = random_rows(rng, len(lengths), k_in, world["n_docs"] + 5)          # docs n_docs .. n_docs + 4: rows of their own
    for g, first, k in ((1, 0, k_in), (3, 0, k_in), (2, 1, min(k_in, 50)), (k_in, 0, 1024)):
        check(sc, hits, n_hits, world["group"], g, first, k, k_in)


@pytest.mark.parametrize("k_in", [1, 65, 129, 257, 1024])
def test_one_group_and_all_distinct(ss_ctx, k_in):
    n_docs = 1100
    body = (np.array([0, 1], np.uint64), np.array([0], np.uint32), np.array([1.0], np.float32))
    sc, ti, bi = make_scorer(ss_ctx, n_docs, body, body, np.ones(n_docs), np.ones(n_docs))
    try:
        rng = np.random.default_rng(k_in)
        hits = random_rows(rng, 2, k_in, n_docs)
        hits["doc"][1] = rng.permutation(n_docs)[:k_in]                       # row 1: distinct docs; row 0: docs repeat
        n_hits = np.array([k_in, k_in], np.int32)
        one = np.full(n_docs, 0x80000000, np.uint32)
        sc.set_doc_groups(one)
        for g in sorted({1, 2, k_in, k_in + 1}):
            o_hits, o_n, o_same, o_kept = check(sc, hits, n_hits, one, g, 0, k_in)
            assert o_n.tolist() == [min(g, k_in)] * 2 == o_kept.tolist() and (o_same[:, :min(g, k_in)] == k_in).all()
            assert o_hits[:, :min(g, k_in)].tobytes() == hits[:, :min(g, k_in)].tobytes()
        # all groups distinct (a table value per doc; then no table value at all): the identity on distinct docs
        for table in (np.arange(n_docs, dtype=np.uint32) * 3000000, np.full(n_docs, NO, np.uint32)):
            sc.set_doc_groups(table)
            o_hits, o_n, o_same, o_kept = check(sc, hits, n_hits, table, 1, 0, k_in)
            assert o_hits[1].tobytes() == hits[1].tobytes() and o_n[1] == k_in == o_kept[1] and (o_same[1] == 1).all()
        assert o_hits[0].tobytes() == hits[0].tobytes()                       # rows of their own: equal docs stay apart
    finally:
        close_all(sc, ti, bi)


def test_group_value_edges_and_the_same_doc_twice(ss_ctx):
    """the high bits of the sort key: table values 0, 1, 2^31 - 1, 2^31 and 2^32 - 2 beside SS_NO_GROUP and docs past the table; rows of
    their own collide neither with each other nor with a table value, whatever their window index"""
    n_docs = 12
    group = np.array(EDGE_VALUES + [NO] + EDGE_VALUES + [NO], np.uint32)      # docs d and d + 6 share a site, docs 5 and 11 have none
    body = (np.array([0, 1], np.uint64), np.array([0], np.uint32), np.array([1.0], np.float32))
    sc, ti, bi = make_scorer(ss_ctx, n_docs, body, body, np.ones(n_docs), np.ones(n_docs))
    try:
        sc.set_doc_groups(group)
        rng = np.random.default_rng(3)
        docs = [[0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, UNKNOWN, 0, 5, 5, 12, 0x80000000, 1, 11],
                [5, 5, 5, 5, 11, 11, 12, 12, UNKNOWN, UNKNOWN, 0x100000, 0, 0, 0, 6, 6, 6, 4, 10, 4, 10]]
        hits = random_rows(rng, 2, 21, 1)
        hits["doc"] = docs
        # finals deliberately out of order, with equal, NaN and -0.0 values: nothing re-sorts, the bytes go through
        hits["final"][0, :6] = [1.0, 7.0, 7.0, float("nan"), -0.0, 0.0]
        n_hits = np.array([21, 21], np.int32)
        for g in (1, 2, 3):
            for first, k in ((0, 21), (4, 5)):
                check(sc, hits, n_hits, group, g, first, k)
        o_hits, o_n, o_same, o_kept = check(sc, hits, n_hits, group, 1, 0, 21)
        # row 0, g = 1: docs 0 - 5 kept, 6 - 10 are their sites' second rows, 11 / 12 / UNKNOWN on their own, 0 again dropped,
        # 5 / 5 / 12 / 2^31 on their own, 1 dropped, 11 on its own
        assert o_hits["doc"][0, :o_n[0]].tolist() == [0, 1, 2, 3, 4, 5, 11, 12, UNKNOWN, 5, 5, 12, 0x80000000, 11]
        assert o_same[0, :o_n[0]].tolist() == [3, 3, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1]
        assert o_hits["doc"][1, :o_n[1]].tolist() == [5, 5, 5, 5, 11, 11, 12, 12, UNKNOWN, UNKNOWN, 0x100000, 0, 4]
    finally:
        close_all(sc, ti, bi)


@pytest.mark.parametrize("k", [1, 50, 1024])
def test_first_and_k(world, scorer, k):
    sc = scorer[0]
    rng = np.random.default_rng(k)
    hits = random_rows(rng, 3, 200, world["n_docs"])
    n_hits = np.array([200, 137, 1], np.int32)
    kept = want(hits, n_hits, world["group"], 2, 0, 200)[3]
    for n_kept in sorted(set(int(x) for x in kept)):
        firsts = {0, n_kept - 1, n_kept, n_kept + 1, max(0, n_kept - (k + 1) // 2), 2 ** 31 - 1}
        for first in sorted(firsts):
            check(sc, hits, n_hits, world["group"], 2, first, k)


def test_random_batch(world, scorer):
    """300 queries: window lengths from {1, 3, 50} and full, group counts from {1, 3, 50, all distinct}"""
    sc = scorer[0]
    rng = np.random.default_rng(9)
    n_q, k_in, n_docs = 300, 64, world["n_docs"]
    hits = random_rows(rng, n_q, k_in, n_docs)
    n_hits = rng.choice(np.array([1, 3, 50, k_in], np.int32), n_q)
    tables = {1: np.full(n_docs, 4, np.uint32), 3: rng.integers(0, 3, n_docs).astype(np.uint32) * 0x7FFFFFFF,
              50: rng.integers(0, 50, n_docs).astype(np.uint32), "all": np.arange(n_docs, dtype=np.uint32)}
    # one table a call: the queries draw their group count by drawing docs from a slice of a table glued from the four
    glued = np.concatenate([tables[1], tables[3] + 100, tables[50] + 1000, tables["all"] + 100000]).astype(np.uint32)
    which = rng.integers(0, 4, n_q)
    hits["doc"] += (which * n_docs).astype(np.uint32)[:, None]
    body = (np.array([0, 1], np.uint64), np.array([0], np.uint32), np.array([1.0], np.float32))
    sc2, ti, bi = make_scorer(sc.ctx, 4 * n_docs, body, body, np.ones(4 * n_docs), np.ones(4 * n_docs))
    try:
        sc2.set_doc_groups(glued)
        for g, first, k in ((1, 0, 64), (2, 0, 50), (2, 50, 50), (5, 3, 7)):
            check(sc2, hits, n_hits, glued, g, first, k)
    finally:
        close_all(sc2, ti, bi)


def test_pointer_placements(ss_ctx, world, scorer):
    import torch
    sc = scorer[0]
    lib = ss_ctx.lib
    rng = np.random.default_rng(4)
    n_q, k_in, g, first, k = 9, 130, 2, 3, 40
    group = world["group"]
    hits = random_rows(rng, n_q, k_in, world["n_docs"] + 2)
    n_hits = rng.integers(0, k_in + 1, n_q).astype(np.int32)
    ref = as_bytes(want(hits, n_hits, group, g, first, k))

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()

    def run(h, n, o, code=0):
        ptr = lambda a: None if a is None else a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data       # noqa: E731
        torch.cuda.synchronize()
        rc = lib.ss_collapse_hits(sc.h, n_q, k_in, ptr(h), ptr(n), g, first, k, ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(o[3]))
        assert rc == code
        ss_ctx.synchronize()
        return [None if a is None else (a.cpu().numpy() if hasattr(a, "cpu") else a).tobytes() for a in o]

    d_hits, d_n = dev(hits), dev(n_hits)
    host_out = lambda: list(outputs(n_q, k))                                 # noqa: E731
    dev_out = lambda: [dev(a) for a in outputs(n_q, k)]                     # noqa: E731
    assert run(d_hits, d_n, dev_out()) == ref                                # all device
    assert run(hits, n_hits, host_out()) == ref                              # all host
    assert run(d_hits, n_hits, dev_out()) == ref                             # mixed inputs, device outputs
    assert run(hits, d_n, host_out()) == ref
    mixed = host_out()
    mixed[0], mixed[3] = dev(mixed[0]), dev(mixed[3])
    assert run(d_hits, d_n, mixed) == ref                                    # device rows and n_kept, host counts and same
    mixed = dev_out()
    mixed[0], mixed[3] = outputs(n_q, k)[0], outputs(n_q, k)[3]
    assert run(hits, d_n, mixed) == ref
    for drop in ((2,), (3,), (2, 3)):                                        # same_out / n_kept_out NULL
        for make in (host_out, dev_out):
            o = make()
            for i in drop:
                o[i] = None
            assert run(d_hits if make is dev_out else hits, d_n, o) == [None if i in drop else ref[i] for i in range(4)]
    # a device n_hits outside [0, k_in] is clamped by the kernel; the same array in host memory is refused
    bad = n_hits.copy()
    bad[0], bad[1], bad[5] = -1, k_in + 5, -2 ** 31
    clamped = as_bytes(want(hits, bad, group, g, first, k, clamp=True))
    assert run(d_hits, dev(bad), dev_out()) == clamped
    assert run(hits, dev(bad), host_out()) == clamped
    o = host_out()
    assert run(hits, bad, o, code=ERR_INVALID) == as_bytes(outputs(n_q, k))
    # the engine wrapper with device arrays returns them as they are
    o = dev_out()
    got = sc.collapse_hits(d_hits, d_n.view(torch.int32), g, k, first=first, k_in=k_in,
                           out=(o[0], o[1].view(torch.int32), o[2].view(torch.int32), o[3].view(torch.int32)))
    assert [a.cpu().numpy().tobytes() for a in got] == ref


def test_refusals_leave_the_outputs_untouched(ss_ctx, world):
    sc, ti, bi = make_scorer(ss_ctx, world["n_docs"], world["title"], world["body"], world["mt"], world["mb"])
    try:
        lib = ss_ctx.lib
        rng = np.random.default_rng(8)
        hits = random_rows(rng, 2, 4, world["n_docs"])
        n_hits = np.array([4, 2], np.int32)
        out = outputs(2, 3)
        untouched = as_bytes(outputs(2, 3))
        q_ptr, q_terms = np.array([0, 1, 3], np.uint32), np.array([0, 1, 2], np.uint32)
        ptr = lambda a: None if a is None else a.ctypes.data       # noqa: E731

        def call(code, handle="sc", n_q=2, k_in=4, h=hits, n=n_hits, g=1, first=0, k=3, o0=out[0], o1=out[1]):
            rc = lib.ss_collapse_hits(sc.h if handle == "sc" else handle, n_q, k_in, ptr(h), ptr(n), g, first, k, ptr(o0), ptr(o1),
                                      ptr(out[2]), ptr(out[3]))
            assert rc == code, (rc, code)
            assert as_bytes(out) == untouched

        def scored(code, handle="sc", n_q=2, qp=q_ptr, k_window=4, g=1, first=0, k=3, o0=out[0], o1=out[1], probs=None):
            rc = lib.ss_score_topk_collapsed(sc.h if handle == "sc" else handle, n_q, ptr(qp), ptr(q_terms), None, ptr(probs), None,
                                             k_window, g, first, k, ptr(o0), ptr(o1), ptr(out[2]), ptr(out[3]))
            assert rc == code, (rc, code)
            assert as_bytes(out) == untouched
        # no table yet
        call(ERR_STATE)
        scored(ERR_STATE)
        with pytest.raises(SpaghettiError) as ei:
            sc.collapse_hits(hits, n_hits, 1, 3, out=out)
        assert ei.value.code == ERR_STATE and as_bytes(out) == untouched
        sc.set_doc_groups(world["group"])
        for fn in (call, scored):
            fn(ERR_INVALID, handle=None)
            fn(ERR_INVALID, n_q=-1)
            fn(ERR_INVALID, g=0)
            fn(ERR_INVALID, first=-1)
            fn(ERR_INVALID, k=0)
            fn(ERR_INVALID, o0=None)
            fn(ERR_INVALID, o1=None)
            fn(ERR_UNSUPPORTED, k=1025)
        call(ERR_INVALID, k_in=0)
        call(ERR_INVALID, h=None)
        call(ERR_INVALID, n=None)
        call(ERR_UNSUPPORTED, k_in=1025)
        call(ERR_INVALID, n=np.array([5, 1], np.int32))
        call(ERR_INVALID, n=np.array([1, -1], np.int32))
        scored(ERR_INVALID, k_window=0)
        scored(ERR_INVALID, qp=None)
        scored(ERR_INVALID, qp=np.array([0, 3, 2], np.uint32))
        scored(ERR_UNSUPPORTED, k_window=1025)
        scored(ERR_STATE, probs=np.ones(2))                                   # topic_probs without a prior
        # hits_out overlapping hits: the same array, and one that starts inside it
        both = np.concatenate([hits.reshape(-1), hits.reshape(-1)])
        before = both.tobytes()
        for off in (0, 1, 7):
            rc = lib.ss_collapse_hits(sc.h, 2, 4, both.ctypes.data, n_hits.ctypes.data, 1, 0, 3, both[off:].ctypes.data, ptr(out[1]),
                                      None, None)
            assert rc == ERR_INVALID and both.tobytes() == before and as_bytes(out) == untouched
        rc = lib.ss_collapse_hits(sc.h, 2, 4, both.ctypes.data, n_hits.ctypes.data, 1, 0, 3, both[8:].ctypes.data, ptr(out[1]), None, None)
        assert rc == 0 and both[:8].tobytes() == before[:320]                 # right behind the input: fine
        out[1][:] = filled(2, np.int32)
        call(0, n_q=0)                                                        # nothing to do: SS_OK, nothing written
        call(0, n_q=0, h=None, n=None, o0=None, o1=None)
        scored(0, n_q=0, qp=np.array([0], np.uint32))
        # the same arguments untouched are accepted, and after clearing the table refused again
        check(sc, hits, n_hits, world["group"], 1, 0, 3)
        sc.set_doc_groups(None)
        call(ERR_STATE)
        scored(ERR_STATE)
    finally:
        close_all(sc, ti, bi)


def tail_and_head_queries(world):
    """head terms (windows of hundreds of rows), tail terms (a few rows), a query of unknown terms only (an empty row)"""
    z_len = np.diff(world["body"][0].astype(np.int64))
    tail = [int(t) for t in np.argsort(z_len)[:3]]
    rows = [[0, 1, 2], [3], [tail[0]], [UNKNOWN, world["n_terms"]], [5, 9, 20, 3], [tail[1], tail[2]], [0], [40, 41, 42, 43, 44, 45]]
    q_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint32)
    return q_ptr, np.array([t for r in rows for t in r], dtype=np.uint32)


@pytest.mark.parametrize("k_window", [1, 50, 1024])
@pytest.mark.parametrize("variant", ["plain", "masked", "prior"])
def test_score_topk_collapsed_equals_score_then_model(world, scorer, k_window, variant):
    sc = scorer[0]
    n_docs, group = world["n_docs"], world["group"]
    q_ptr, q_terms = tail_and_head_queries(world)
    n_q = len(q_ptr) - 1
    rng = np.random.default_rng(31)
    mask_id = probs = None
    if variant == "masked":
        sc.set_doc_masks(engine.pack_doc_masks(rng.random((2, n_docs)) < 0.5, n_docs))
        mask_id = np.array([0, -1, 1, 0, 1, -1, 0, 1], np.int32)
    if variant == "prior":
        sc.set_prior(rng.random((3, n_docs)))
        probs = rng.random((n_q, 3))
    rows, n_rows = sc.score_topk_masked(q_ptr, q_terms, mask_id, k_window, topic_probs=probs)
    assert n_rows[3] == 0 and (k_window == 1 or 0 < n_rows.min(initial=99, where=n_rows > 0) < n_rows.max())
    if k_window == 1024:
        assert n_rows.max() < k_window                                       # every window shorter than k_window
    for g, first, k in ((1, 0, 50), (2, 0, 50), (2, 50, 50), (3, 2, 1024), (2, 1, 1)):
        got = sc.score_topk_collapsed(q_ptr, q_terms, k_window, g, k, first=first, topic_probs=probs, mask_id=mask_id,
                                      out=outputs(n_q, k))
        assert as_bytes(got) == as_bytes(want(rows, n_rows, group, g, first, k)), (g, first, k)
    if k_window == 50 and variant == "plain":
        assert (got[3] < n_rows).any()                                       # something was collapsed at all


def test_turns_come_round_and_chain_into_explain(ss_ctx, world, scorer):
    """Seven score-and-collapse calls back to back with device outputs, more than twice the scorer's turns, each into buffers of its
    own and each followed by ss_explain_hits on its device rows; nothing waits until the one synchronise at the end.  A turn's rows
    must outlive the collapse kernel that reads them: the calls alternate between two batches whose windows differ."""
    import torch
    from tests import explain_model as xm
    sc = scorer[0]
    lib = ss_ctx.lib
    q_ptr, q_terms = tail_and_head_queries(world)
    n_q = len(q_ptr) - 1
    qp2 = np.array([0, 2, 3, 6], np.uint32)
    qt2 = np.array([7, 8, 60, 1, 2, 3], np.uint32)
    k_window, g, k, t_stride = 300, 2, 20, 6
    rounds = []
    for r in range(7):
        qp, qt = (q_ptr, q_terms) if r % 2 == 0 else (qp2, qt2)
        nq = len(qp) - 1
        rounds.append({"qp": qp, "qt": qt, "nq": nq, "first": 5 * (r // 2),
                       "hits": torch.full((nq * k * 40,), FILL, dtype=torch.uint8, device="cuda"),
                       "n": torch.full((nq * 4,), FILL, dtype=torch.uint8, device="cuda"),
                       "same": torch.full((nq * k * 4,), FILL, dtype=torch.uint8, device="cuda"),
                       "kept": torch.full((nq * 4,), FILL, dtype=torch.uint8, device="cuda"),
                       "exp": torch.full((nq * k * t_stride * 16,), FILL, dtype=torch.uint8, device="cuda")})
    torch.cuda.synchronize()
    for c in rounds:
        rc = lib.ss_score_topk_collapsed(sc.h, c["nq"], c["qp"].ctypes.data, c["qt"].ctypes.data, None, None, None, k_window, g,
                                         c["first"], k, c["hits"].data_ptr(), c["n"].data_ptr(), c["same"].data_ptr(), c["kept"].data_ptr())
        assert rc == 0
        rc = lib.ss_explain_hits(sc.h, c["nq"], c["qp"].ctypes.data, c["qt"].ctypes.data, k, c["hits"].data_ptr(), c["n"].data_ptr(),
                                 t_stride, c["exp"].data_ptr())
        assert rc == 0
    ss_ctx.synchronize()
    for r, c in enumerate(rounds):
        rows, n_rows = sc.score_topk(c["qp"], c["qt"], k_window)
        ref = want(rows, n_rows, world["group"], g, c["first"], k)
        got = [c[name].cpu().numpy() for name in ("hits", "n", "same", "kept")]
        assert [a.tobytes() for a in got] == as_bytes(ref), r
        exp = filled((c["nq"], k, t_stride), engine.TERM_MATCH_DTYPE)
        exp = sc.explain_hits(c["qp"], c["qt"], ref[0], ref[1], t_stride=t_stride, out=exp)
        assert c["exp"].cpu().numpy().tobytes() == exp.tobytes(), r
        assert exp.tobytes() == xm.explain_ref(world["title"], world["body"], world["n_docs"], c["qp"], c["qt"], ref[0]["doc"], ref[1],
                                               t_stride, fill=FILL).tobytes()
    assert any(int(c["n"].view(torch.int32).sum()) > 0 for c in rounds)
