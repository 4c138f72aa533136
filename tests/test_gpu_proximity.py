"""GPU parity: term proximity (ss_hit_proximity, ss_rerank_hits_by_proximity, ss_score_topk_proximity) vs the numpy model
(tests/proximity_model.py).  Every comparison is bit-exact: tobytes() on whole output arrays that start from 0xA5 bytes, so an entry
a call must not write is checked with the ones it must.  Every case runs under "proximity.lds_events" = default, 16 and 1 and must give
identical bytes: the smallest settings at which the LDS path, its padding to a power of two and the global-memory path each run.
"""
import numpy as np
import pytest

from spaghettisearch_amd import SpaghettiError, engine
from tests import proximity_model as xm
from tests.passage_model import body_lists
from tests.test_gpu_passage import made_up, queries
from tests.test_gpu_score import close_all, make_scorer
from tests.test_passage_cpu import GOLDEN, UNKNOWN, random_positions
from tests.test_proximity_cpu import ABC, HAND_CASES, NAMES, hand_world

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_OOM, ERR_STATE, ERR_UNSUPPORTED = 1, 4, 6, 7
FILL = 0xA5
CAPS = (None, 16, 1)
NAN, INF = float("nan"), float("inf")


def prefilled(dtype, *shape):
    n = int(np.prod(shape))
    return np.frombuffer(bytes([FILL]) * (n * np.dtype(dtype).itemsize), dtype=dtype).reshape(shape).copy()


def untouched(*arrays):
    return all((a.view(np.uint8) == FILL).all() for a in arrays)


def under_caps(ss_ctx, call):
    """call() under every cap -> its results' bytes, after asserting that the three are the same"""
    got = []
    for cap in CAPS:
        with ss_ctx.options(proximity__lds_events=cap):
            r = call()
        got.append(tuple(a.tobytes() for a in (r if isinstance(r, tuple) else (r,))))
    assert got[0] == got[1] == got[2]
    return got[0]


def proximity(sc, q_ptr, q_terms, hits, n_hits):
    n_q, k = hits.shape
    return sc.hit_proximity(q_ptr, q_terms, hits, n_hits, out=prefilled(engine.PROXIMITY_DTYPE, n_q, k))


def rerank_out(n_q, k):
    return (prefilled(engine.HIT_DTYPE, n_q, k), prefilled(np.int32, n_q), prefilled(np.float64, n_q, k), prefilled(engine.PROXIMITY_DTYPE, n_q, k))


def rerank(sc, q_ptr, q_terms, hits, n_hits, w_rank, w_prox, first, k):
    return sc.rerank_by_proximity(q_ptr, q_terms, hits, n_hits, k, w_rank, w_prox, first, out=rerank_out(hits.shape[0], k))


def model_bytes(ref, n_q):
    """the model's four arrays as the bytes the library must give: n_hits_out is written whole"""
    return tuple(a.tobytes() for a in ref)


@pytest.fixture(scope="module")
def world():
    """The golden 300 x 80 tables with their stored weights, body positions with every 9th list long (70 - 200 values), and the batch
    of test_gpu_passage.py: 1-, 3- and 12-token queries, a duplicated token, unknown ids, one query of unknown terms only."""
    z = np.load(GOLDEN)
    n_docs, n_terms = int(z["n_docs"]), len(z["b_ptr"]) - 1
    rows = [[3], [0, 1, 2], [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11], [UNKNOWN, n_terms], [70, 5, 70],
            [79, 40, UNKNOWN, 1, 1, n_terms, 33, 2, 60, 0, 79, 12], [50]]
    q_ptr, q_terms = queries(rows)
    return {"n_docs": n_docs, "n_terms": n_terms, "title": (z["t_ptr"], z["t_doc"], z["t_w"]), "body": (z["b_ptr"], z["b_doc"], z["b_w"]),
            "mt": z["t_mag"], "mb": z["b_mag"], "bpos": random_positions(len(z["b_doc"]), 8, long_every=9), "q_ptr": q_ptr,
            "q_terms": q_terms, "rows": rows, "ref": {}}


@pytest.fixture()
def scorer(ss_ctx, world):
    sc, ti, bi = make_scorer(ss_ctx, world["n_docs"], world["title"], world["body"], world["mt"], world["mb"])
    bi.set_positions(*world["bpos"])
    yield sc, ti, bi
    close_all(sc, ti, bi)


def model(world, hits, n_hits):
    return xm.proximity_ref(world["body"], world["n_docs"], world["q_ptr"], world["q_terms"], hits["doc"], n_hits, body_pos=world["bpos"], fill=FILL)


def model_rerank(world, hits, n_hits, w_rank, w_prox, first, k):
    return xm.rerank_ref(world["body"], world["n_docs"], world["q_ptr"], world["q_terms"], hits, n_hits, w_rank, w_prox, first, k,
                         body_pos=world["bpos"], fill=FILL)


def world_rows(world, sc, k):
    """(hits, n_hits, the model's entries as bytes) of the world's batch at k: computed once per module"""
    if k not in world["ref"]:
        hits, n_hits = sc.score_topk(world["q_ptr"], world["q_terms"], k)
        world["ref"][k] = (hits, n_hits, model(world, hits, n_hits).tobytes())
    return world["ref"][k]


@pytest.mark.parametrize("k", [1, 10, 40])
def test_rows_of_score_topk_equal_the_model(ss_ctx, world, scorer, k):
    sc, ti, bi = scorer
    hits, n_hits, want = world_rows(world, sc, k)
    assert n_hits[3] == 0 and n_hits[2] == k
    got, = under_caps(ss_ctx, lambda: proximity(sc, world["q_ptr"], world["q_terms"], hits, n_hits))
    assert got == want
    ent = np.frombuffer(got, dtype=engine.PROXIMITY_DTYPE).reshape(len(n_hits), k)
    assert ent[3].tobytes() == bytes([FILL]) * (k * 24)                       # the query without hits: nothing is written
    assert (ent["n_present"][2, :k] > 1).any()
    if k == 40:
        lists = body_lists(world["body"], world["bpos"])
        n = [sum(len(lists.get((t, int(d)), ())) for t in set(world["rows"][q])) for q in range(len(n_hits)) for d in hits["doc"][q, :n_hits[q]]]
        # cap 16: both sides, and lengths that are no power of two below it; cap 1: lists of one value and longer ones; default: all in the LDS
        assert sum(x <= 1 for x in n) > 0 and sum(x in (3, 5, 6, 7, 9, 10, 11, 12, 13) for x in n) > 5 and sum(x > 16 for x in n) > 5
        assert max(n) <= 512 and sum(x > 64 and x & (x - 1) for x in n) > 5


def test_hand_world_and_known_answer(ss_ctx):
    n_docs, title, body, pos = hand_world()
    sc, ti, bi = make_scorer(ss_ctx, n_docs, title, body, np.ones(n_docs), np.ones(n_docs))
    try:
        def run(with_pos):
            for d, c in enumerate(HAND_CASES):
                q_ptr, q_terms = queries([c["tokens"]])
                hits, n_hits = made_up([[d]], k=2)
                want = xm.proximity_ref(body, n_docs, q_ptr, q_terms, hits["doc"], n_hits, body_pos=pos if with_pos else None, fill=FILL)
                got, = under_caps(ss_ctx, lambda: proximity(sc, q_ptr, q_terms, hits, n_hits))
                assert got == want.tobytes(), c["name"]
                e = np.frombuffer(got, dtype=engine.PROXIMITY_DTYPE)
                assert e[1].tobytes() == bytes([FILL]) * 24
                if with_pos:
                    assert np.array(c["want"][:2], np.float32).tobytes() == e[0]["start"].tobytes() + e[0]["end"].tobytes(), c["name"]
                    assert (int(e[0]["n_present"]), int(e[0]["n_occ"]), int(e[0]["token_mask"])) == c["want"][2:], c["name"]
                else:
                    assert e[0].tobytes() == bytes(24)
        run(False)                                                            # no positions table: 24 zero bytes, written
        bi.set_positions(*pos)
        run(True)
        x, y, z, w = (NAMES.index(n) for n in "XYZW")
        q_ptr, q_terms = queries([ABC, [1, 0, 1], [0]])
        # made-up rows: docs at and past n_docs between real ones, slots behind n_hits naming a doc with a span
        hits, n_hits = made_up([[x, n_docs, y, UNKNOWN, z], [y, y], []], k=6)
        hits["doc"][:, 5] = x
        hits["doc"][2, :] = x
        got, = under_caps(ss_ctx, lambda: proximity(sc, q_ptr, q_terms, hits, n_hits))
        assert got == xm.proximity_ref(body, n_docs, q_ptr, q_terms, hits["doc"], n_hits, body_pos=pos, fill=FILL).tobytes()
        e = np.frombuffer(got, dtype=engine.PROXIMITY_DTYPE).reshape(3, 6)
        assert e[0, 1].tobytes() == bytes(24) and e[0, 3].tobytes() == bytes(24) and e["n_present"][0, [0, 2, 4]].tolist() == [3, 2, 1]
        assert e[0, 5].tobytes() == bytes([FILL]) * 24 and e[2].tobytes() == bytes([FILL]) * (6 * 24) and int(e["token_mask"][1, 0]) == 0b111
        # the known answer: the window (W, Z, Y, X) with w_rank = 0, w_prox = 1 comes back as Y, X, W, Z
        q_ptr, q_terms = queries([ABC])
        hits, n_hits = made_up([[w, z, y, x]])
        hits["final"][0] = [0.9, 0.8, 0.7, 0.6]
        want = xm.rerank_ref(body, n_docs, q_ptr, q_terms, hits, n_hits, 0.0, 1.0, 0, 4, body_pos=pos, fill=FILL)
        got = under_caps(ss_ctx, lambda: rerank(sc, q_ptr, q_terms, hits, n_hits, 0.0, 1.0, 0, 4))
        assert got == model_bytes(want, 1)
        assert np.frombuffer(got[0], dtype=engine.HIT_DTYPE)["doc"].tolist() == [y, x, w, z]
        assert np.frombuffer(got[2], dtype=np.float64).tolist() == [2.0 / 3.0, 2.0 / 3.0, 0.0, 0.0]
    finally:
        close_all(sc, ti, bi)


def test_a_doc_of_six_thousand_values(ss_ctx):
    """one doc whose three terms hold 2,000 values each (more than any cap the option admits), beside a doc of 3 x 170 (just under the
    default cap of 512: the LDS sort at its full size) and one of 3 x 171 (just over)"""
    from tests.test_passage_cpu import positions_of
    from tests.test_related_terms_cpu import table_of
    rng = np.random.default_rng(17)
    sizes = [2000, 170, 171]
    lists = []
    for t in range(3):
        for n in sizes:
            vals = rng.integers(0, 30000, size=n).astype(float)
            vals[rng.random(n) < 0.1] = -100.0
            lists.append(vals.tolist())
    body = table_of([{0: 1.0, 1: 1.0, 2: 1.0} for _ in sizes], 3)
    title = table_of([{} for _ in sizes], 3)
    pos = positions_of(lists)
    sc, ti, bi = make_scorer(ss_ctx, 3, title, body, np.ones(3), np.ones(3))
    try:
        bi.set_positions(*pos)
        hits, n_hits = made_up([[0, 1, 2]])
        q_ptr, q_terms = queries([[2, 0, 1, 0]])
        got = proximity(sc, q_ptr, q_terms, hits, n_hits)
        want = xm.proximity_ref(body, 3, q_ptr, q_terms, hits["doc"], n_hits, body_pos=pos, fill=FILL)
        assert got.tobytes() == want.tobytes()
        assert (got["n_present"][0] == 3).all() and (got["token_mask"][0] == 0b1111).all() and (got["n_occ"][0] >= 3).all()
    finally:
        close_all(sc, ti, bi)


def test_rerank_pages_and_edges(ss_ctx, world, scorer):
    sc, ti, bi = scorer
    n_docs = world["n_docs"]
    hits, n_hits, _ = world_rows(world, sc, 40)
    n_q = len(n_hits)
    # paging: a whole window, first + k > n, first >= n, k = 1
    for w_rank, w_prox, first, k in ((1.0, 0.5, 0, 40), (1.0, 0.5, 35, 10), (1.0, 0.5, 40, 3), (0.25, 2.0, 2, 1)):
        want = model_rerank(world, hits, n_hits, w_rank, w_prox, first, k)
        got = under_caps(ss_ctx, lambda: rerank(sc, world["q_ptr"], world["q_terms"], hits, n_hits, w_rank, w_prox, first, k))
        assert got == model_bytes(want, n_q), (first, k)
        assert want[1].tolist() == [min(max(int(n) - first, 0), k) for n in n_hits]
    # w_prox == 0 and w_rank > 0 on rows in FinalRank order: the window itself
    got = rerank(sc, world["q_ptr"], world["q_terms"], hits, n_hits, 3.0, 0.0, 0, 40)
    assert all(got[0][q, :n_hits[q]].tobytes() == hits[q, :n_hits[q]].tobytes() for q in range(n_q)) and got[1].tolist() == n_hits.tolist()
    # w_rank == 0: bonus descending, then window order
    got = rerank(sc, world["q_ptr"], world["q_terms"], hits, n_hits, 0.0, 1.0, 0, 40)
    ent = np.frombuffer(world["ref"][40][2], dtype=engine.PROXIMITY_DTYPE).reshape(n_q, 40)
    moved = False
    for q in range(n_q):
        n, big_t = int(n_hits[q]), len(set(world["rows"][q]))
        bonus = [float(xm.bonus_of(ent[q, j], big_t)) for j in range(n)]
        order = sorted(range(n), key=lambda j: (-bonus[j], j))
        assert got[0][q, :n].tobytes() == hits[q, order].tobytes() and got[2][q, :n].tolist() == [bonus[j] for j in order]
        moved = moved or order != list(range(n))
    assert moved                                                              # it re-orders
    # made-up windows: docs outside the table, repeated docs, NaN, -0.0 and infinite finals; a negative weight
    odd = hits.copy()
    odd["doc"][1, [2, 7]] = [n_docs, UNKNOWN]
    odd["doc"][1, 5] = odd["doc"][1, 4]
    odd["final"][1, [0, 3, 9, 11, 12]] = [NAN, -0.0, NAN, INF, -INF]
    odd["doc"][2, :6] = odd["doc"][2, 0]
    odd["final"][2, :6] = 0.5
    odd["final"][0] = -0.0
    odd["_pad"][4] = 0xDEADBEEF
    for w_rank, w_prox in ((1.0, 0.5), (1.0, -1.0), (0.0, 1.0), (-1.0, 0.0)):
        want = model_rerank(world, odd, n_hits, w_rank, w_prox, 0, 40)
        got = under_caps(ss_ctx, lambda: rerank(sc, world["q_ptr"], world["q_terms"], odd, n_hits, w_rank, w_prox, 0, 40))
        assert got == model_bytes(want, n_q), (w_rank, w_prox)
    # NaN canonicalisation: a NaN of another payload in, 0x7FF8000000000000 out, and for the rows outside the table too
    odd["final"].view(np.uint64)[1, 0] = 0xFFF0000000000123
    got = rerank(sc, world["q_ptr"], world["q_terms"], odd, n_hits, 1.0, 0.5, 0, 40)
    assert got[0].tobytes() == model_rerank(world, odd, n_hits, 1.0, 0.5, 0, 40)[0].tobytes()
    n1 = int(n_hits[1])
    assert got[2].view(np.uint64)[1, n1 - 4:n1].tolist() == [xm.NAN_BITS] * 4 and got[3][1, n1 - 2:n1].tobytes() == bytes(48)
    assert got[0]["final"].view(np.uint64)[1, n1 - 4] == 0xFFF0000000000123    # the row itself is a copy


def test_host_arrays_device_tensors_and_the_scored_form(ss_ctx, world, scorer):
    import torch
    sc, ti, bi = scorer
    k_in, first, k = 40, 3, 10
    hits, n_hits, want_ent = world_rows(world, sc, k_in)
    n_q = len(n_hits)
    want = model_bytes(model_rerank(world, hits, n_hits, 1.0, 0.5, first, k), n_q)
    dev = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()   # noqa: E731
    filled = lambda n: torch.full((n,), FILL, dtype=torch.uint8, device="cuda")   # noqa: E731
    d_hits, d_n = dev(hits), torch.from_numpy(n_hits.copy()).cuda()
    # entries: everything on the device, and mixed
    d_out = filled(n_q * k_in * 24)
    sc.hit_proximity(world["q_ptr"], world["q_terms"], d_hits, d_n, out=d_out, k=k_in)
    assert d_out.cpu().numpy().tobytes() == want_ent
    assert sc.hit_proximity(world["q_ptr"], world["q_terms"], d_hits, n_hits, out=prefilled(engine.PROXIMITY_DTYPE, n_q, k_in), k=k_in).tobytes() == want_ent
    # the re-rank: everything on the device; host scores with device entries and the other way round; without the optional outputs
    d_o = (filled(n_q * k * 40), torch.full((n_q,), -1, dtype=torch.int32, device="cuda"),
           torch.from_numpy(prefilled(np.float64, n_q, k)).cuda(), filled(n_q * k * 24))
    sc.rerank_by_proximity(world["q_ptr"], world["q_terms"], d_hits, d_n, k, 1.0, 0.5, first, k_in=k_in, out=d_o)
    assert tuple(t.cpu().numpy().tobytes() for t in d_o) == want
    o = rerank_out(n_q, k)
    mixed = sc.rerank_by_proximity(world["q_ptr"], world["q_terms"], hits, d_n, k, 1.0, 0.5, first, out=(o[0], o[1], o[2], filled(n_q * k * 24)))
    assert tuple(a.tobytes() for a in mixed[:3]) == want[:3] and mixed[3].cpu().numpy().tobytes() == want[3]
    o = rerank_out(n_q, k)
    d_sc = torch.from_numpy(prefilled(np.float64, n_q, k)).cuda()
    mixed = sc.rerank_by_proximity(world["q_ptr"], world["q_terms"], d_hits, n_hits, k, 1.0, 0.5, first, k_in=k_in, out=(filled(n_q * k * 40), o[1], d_sc, o[3]))
    assert (mixed[0].cpu().numpy().tobytes(), mixed[1].tobytes(), mixed[2].cpu().numpy().tobytes(), mixed[3].tobytes()) == want
    o = rerank_out(n_q, k)
    bare = sc.rerank_by_proximity(world["q_ptr"], world["q_terms"], hits, n_hits, k, 1.0, 0.5, first, out=(o[0], o[1], None, None))
    assert (bare[0].tobytes(), bare[1].tobytes()) == want[:2] and bare[2] is None and bare[3] is None
    # a device n_hits outside [0, k_in] is clamped by the kernels (host: refused, see the refusals test)
    d_bad = torch.tensor([k_in + 5, -3] + [0] * (n_q - 2), dtype=torch.int32, device="cuda")
    clamped = np.array([k_in, 0] + [0] * (n_q - 2), np.int32)
    torch.cuda.synchronize()
    got = sc.hit_proximity(world["q_ptr"], world["q_terms"], hits, d_bad, out=prefilled(engine.PROXIMITY_DTYPE, n_q, k_in))
    assert got.tobytes() == model(world, hits, clamped).tobytes()
    got = sc.rerank_by_proximity(world["q_ptr"], world["q_terms"], hits, d_bad, k, 1.0, 0.5, first, out=rerank_out(n_q, k))
    assert tuple(a.tobytes() for a in got) == model_bytes(model_rerank(world, hits, clamped, 1.0, 0.5, first, k), n_q)
    # ss_score_topk_proximity equals score-then-rerank, byte for byte: host outputs, device outputs, with a mask and a query_len
    got = under_caps(ss_ctx, lambda: sc.score_topk_proximity(world["q_ptr"], world["q_terms"], k_in, k, 1.0, 0.5, first, out=rerank_out(n_q, k)))
    assert got == want
    d_o = (filled(n_q * k * 40), torch.full((n_q,), -1, dtype=torch.int32, device="cuda"),
           torch.from_numpy(prefilled(np.float64, n_q, k)).cuda(), filled(n_q * k * 24))
    for _ in range(4):                                                        # more rounds than the scorer has turns, nothing waited for
        assert ss_ctx.lib.ss_score_topk_proximity(sc.h, n_q, world["q_ptr"].ctypes.data, world["q_terms"].ctypes.data, None, None, None, k_in, 1.0,
                                                  0.5, first, k, *(t.data_ptr() for t in d_o)) == 0
    ss_ctx.synchronize()
    assert tuple(t.cpu().numpy().tobytes() for t in d_o) == want
    words = np.zeros((1, (world["n_docs"] + 31) // 32), np.uint32)
    words[0, ::2] = 0xFFFF00FF
    sc.set_doc_masks(words)
    mask_id = np.array([0, -1, 0, 0, -1, 0, 0], np.int32)
    qlen = np.array([1, 3, 12, 2, 2, 9, 1], np.int32)
    m_hits, m_n = sc.score_topk_masked(world["q_ptr"], world["q_terms"], mask_id, k_in, query_len=qlen)
    got = sc.score_topk_proximity(world["q_ptr"], world["q_terms"], k_in, k, 0.5, 1.5, 0, query_len=qlen, mask_id=mask_id, out=rerank_out(n_q, k))
    assert tuple(a.tobytes() for a in got) == model_bytes(model_rerank(world, m_hits, m_n, 0.5, 1.5, 0, k), n_q)
    assert m_hits.tobytes() != hits.tobytes()


def test_refusals_leave_the_outputs_untouched(ss_ctx, world, scorer):
    sc, ti, bi = scorer
    lib = ss_ctx.lib
    q_ptr, q_terms = queries([[0, 1, 2], [3]])
    hits, n_hits = sc.score_topk(q_ptr, q_terms, 4)
    out = prefilled(engine.PROXIMITY_DTYPE, 2, 4)
    ptr = lambda a: None if a is None else a.ctypes.data       # noqa: E731
    long_q = (np.array([0, 65, 66], np.uint32), np.zeros(66, np.uint32))

    def entries(code, n_q=2, qp=q_ptr, qt=q_terms, k=4, h=hits, n=n_hits, o=out):
        rc = lib.ss_hit_proximity(sc.h, n_q, ptr(qp), ptr(qt), k, ptr(h), ptr(n), ptr(o))
        assert rc == code, (rc, code)
        assert untouched(out)
    assert lib.ss_hit_proximity(None, 2, ptr(q_ptr), ptr(q_terms), 4, ptr(hits), ptr(n_hits), ptr(out)) == ERR_INVALID and untouched(out)
    entries(ERR_INVALID, o=None)
    entries(ERR_INVALID, n_q=-1)
    entries(ERR_INVALID, k=0)
    entries(ERR_INVALID, qp=None)
    entries(ERR_INVALID, qp=np.array([0, 3, 2], np.uint32))
    entries(ERR_INVALID, qt=None)
    entries(ERR_INVALID, h=None)
    entries(ERR_INVALID, n=None)
    entries(ERR_UNSUPPORTED, k=1025)
    entries(ERR_UNSUPPORTED, qp=long_q[0], qt=long_q[1])                                         # a query of 65 tokens
    entries(ERR_UNSUPPORTED, n_q=1 << 21, k=1024, qp=np.zeros((1 << 21) + 1, np.uint32))          # 2^31 entries
    entries(ERR_INVALID, n=np.array([5, 1], np.int32))
    entries(ERR_INVALID, n=np.array([1, -1], np.int32))
    entries(0, n_q=0)                                                   # nothing to do: SS_OK, nothing written
    with pytest.raises(SpaghettiError) as ei:
        sc.hit_proximity(q_ptr, q_terms, hits, np.array([5, 1], np.int32), out=out)
    assert ei.value.code == ERR_INVALID and untouched(out)
    o = rerank_out(2, 3)

    def paged(code, n_q=2, qp=q_ptr, qt=q_terms, k_in=4, h=hits, n=n_hits, w_rank=1.0, w_prox=1.0, first=0, k=3, oh=o[0], on=o[1], osc=o[2], opx=o[3]):
        rc = lib.ss_rerank_hits_by_proximity(sc.h, n_q, ptr(qp), ptr(qt), k_in, ptr(h), ptr(n), w_rank, w_prox, first, k, ptr(oh), ptr(on),
                                             ptr(osc), ptr(opx))
        assert rc == code, (rc, code)
        assert untouched(*o)
    assert lib.ss_rerank_hits_by_proximity(None, 2, ptr(q_ptr), ptr(q_terms), 4, ptr(hits), ptr(n_hits), 1.0, 1.0, 0, 3, *(ptr(a) for a in o)) == ERR_INVALID
    paged(ERR_INVALID, n_q=-1)
    paged(ERR_INVALID, k_in=0)
    paged(ERR_INVALID, k=0)
    paged(ERR_INVALID, first=-1)
    paged(ERR_UNSUPPORTED, k_in=1025)
    paged(ERR_UNSUPPORTED, k=1025)
    paged(ERR_INVALID, h=None)
    paged(ERR_INVALID, n=None)
    paged(ERR_INVALID, oh=None)
    paged(ERR_INVALID, on=None)
    both = prefilled(engine.HIT_DTYPE, 2, 8)
    rc = lib.ss_rerank_hits_by_proximity(sc.h, 2, ptr(q_ptr), ptr(q_terms), 4, both.ctypes.data, ptr(n_hits), 1.0, 1.0, 0, 3,
                                         both.ctypes.data + 7 * 40, ptr(o[1]), None, None)
    assert rc == ERR_INVALID and untouched(both, *o)                      # hits_out overlaps hits
    paged(ERR_INVALID, qp=None)
    paged(ERR_INVALID, qp=np.array([0, 3, 2], np.uint32))
    paged(ERR_INVALID, qt=None)
    paged(ERR_UNSUPPORTED, qp=long_q[0], qt=long_q[1])
    paged(ERR_INVALID, n=np.array([5, 1], np.int32))
    for bad in (NAN, INF, -INF):
        paged(ERR_INVALID, w_rank=bad)
        paged(ERR_INVALID, w_prox=bad)
    paged(0, n_q=0)

    def scored(code, n_q=2, qp=q_ptr, qt=q_terms, probs=None, mask=None, k_window=4, w_rank=1.0, w_prox=1.0, first=0, k=3, oh=o[0], on=o[1]):
        rc = lib.ss_score_topk_proximity(sc.h, n_q, ptr(qp), ptr(qt), None, ptr(probs), ptr(mask), k_window, w_rank, w_prox, first, k, ptr(oh),
                                         ptr(on), ptr(o[2]), ptr(o[3]))
        assert rc == code, (rc, code)
        assert untouched(*o)
    assert lib.ss_score_topk_proximity(None, 2, ptr(q_ptr), ptr(q_terms), None, None, None, 4, 1.0, 1.0, 0, 3, *(ptr(a) for a in o)) == ERR_INVALID
    scored(ERR_INVALID, n_q=-1)
    scored(ERR_INVALID, k_window=0)
    scored(ERR_INVALID, k=0)
    scored(ERR_INVALID, first=-1)
    scored(ERR_UNSUPPORTED, k_window=1025)
    scored(ERR_INVALID, qp=None)
    scored(ERR_INVALID, qp=np.array([0, 3, 2], np.uint32))
    scored(ERR_INVALID, oh=None)
    scored(ERR_INVALID, on=None)
    scored(ERR_INVALID, w_prox=NAN)
    scored(ERR_INVALID, w_rank=INF)
    scored(ERR_UNSUPPORTED, qp=long_q[0], qt=long_q[1])
    scored(ERR_STATE, probs=np.ones(2, np.float64))                       # topic_probs without a prior
    scored(ERR_INVALID, mask=np.array([0, 3], np.int32))                  # the scoring call's own check: no mask registered
    scored(0, n_q=0)
    # a query of exactly 64 tokens is accepted, and the same arguments untouched work
    q64 = queries([[t % 7 for t in range(64)], [3]])
    want = xm.proximity_ref(world["body"], world["n_docs"], q64[0], q64[1], hits["doc"], n_hits, body_pos=world["bpos"], fill=FILL)
    assert proximity(sc, q64[0], q64[1], hits, n_hits).tobytes() == want.tobytes()
    got = rerank(sc, q_ptr, q_terms, hits, n_hits, 1.0, 1.0, 0, 3)
    want = xm.rerank_ref(world["body"], world["n_docs"], q_ptr, q_terms, hits, n_hits, 1.0, 1.0, 0, 3, body_pos=world["bpos"], fill=FILL)
    assert tuple(a.tobytes() for a in got) == model_bytes(want, 2)
