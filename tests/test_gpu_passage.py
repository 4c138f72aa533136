"""GPU parity: "best passage per hit" (ss_best_passages) vs the numpy model (tests/passage_model.passages_ref).  Every comparison
is bit-exact: tobytes() on whole output arrays that start from 0xA5 bytes, so an entry the call must not write is checked with the
ones it must.
"""
import numpy as np
import pytest

from spaghettisearch_amd import SpaghettiError, engine
from tests import passage_model as pm
from tests.test_gpu_score import close_all, make_scorer
from tests.test_passage_cpu import GOLDEN, HAND_CASES, UNKNOWN, hand_world, positions_of, random_positions
from tests.test_related_terms_cpu import table_of

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = 1, 7
FILL = 0xA5


def prefilled(n_q, k):
    return np.frombuffer(bytes([FILL]) * (n_q * k * 24), dtype=engine.PASSAGE_DTYPE).reshape(n_q, k).copy()


def passages(sc, q_ptr, q_terms, hits, n_hits, width):
    n_q, k = hits.shape
    return sc.best_passages(q_ptr, q_terms, hits, n_hits, width, out=prefilled(n_q, k))


def made_up(docs_rows, k=None):
    """lists of doc ids -> (hits [n_q][k] with nothing but .doc set, n_hits); slots behind a row's last hit name doc 0"""
    k = k or max(1, max(len(r) for r in docs_rows))
    hits = np.zeros((len(docs_rows), k), dtype=engine.HIT_DTYPE)
    for q, r in enumerate(docs_rows):
        hits["doc"][q, :len(r)] = r
    return hits, np.array([len(r) for r in docs_rows], np.int32)


def queries(rows):
    q_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint32)
    return q_ptr, np.array([t for r in rows for t in r], dtype=np.uint32)


@pytest.fixture(scope="module")
def world():
    """The golden 300 x 80 tables with their stored weights, body positions with every 9th list long (70 - 200 values: a hit
    holds from no value to a few hundred under its query's terms), and a batch that mixes 1-, 3- and 12-token queries: head terms,
    a duplicated token, unknown ids, and one query of unknown terms only (no hits)."""
    z = np.load(GOLDEN)
    n_docs, n_terms = int(z["n_docs"]), len(z["b_ptr"]) - 1
    rows = [[3], [0, 1, 2], [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11], [UNKNOWN, n_terms], [70, 5, 70],
            [79, 40, UNKNOWN, 1, 1, n_terms, 33, 2, 60, 0, 79, 12], [50]]
    q_ptr, q_terms = queries(rows)
    return {"n_docs": n_docs, "n_terms": n_terms, "title": (z["t_ptr"], z["t_doc"], z["t_w"]), "body": (z["b_ptr"], z["b_doc"], z["b_w"]),
            "mt": z["t_mag"], "mb": z["b_mag"], "bpos": random_positions(len(z["b_doc"]), 8, long_every=9), "q_ptr": q_ptr,
            "q_terms": q_terms, "ref": {}}


@pytest.fixture()
def scorer(ss_ctx, world):
    sc, ti, bi = make_scorer(ss_ctx, world["n_docs"], world["title"], world["body"], world["mt"], world["mb"])
    bi.set_positions(*world["bpos"])
    yield sc, ti, bi
    close_all(sc, ti, bi)


def model(world, q_ptr, q_terms, hits, n_hits, width):
    return pm.passages_ref(world["body"], world["n_docs"], q_ptr, q_terms, hits["doc"], n_hits, width, body_pos=world["bpos"], fill=FILL)


def world_rows(world, sc, k, width):
    """(hits, n_hits, the model's bytes) of the world's batch at k and width: computed once per module"""
    if (k, width) not in world["ref"]:
        hits, n_hits = sc.score_topk(world["q_ptr"], world["q_terms"], k)
        world["ref"][(k, width)] = (hits, n_hits, model(world, world["q_ptr"], world["q_terms"], hits, n_hits, width).tobytes())
    return world["ref"][(k, width)]


def raw_lengths(world, q_ptr, q_terms, hits, n_hits):
    """per written entry the number of position values under the query's distinct terms: what the kernel compares with its cap"""
    lists = pm.body_lists(world["body"], world["bpos"])
    out = []
    for q in range(len(q_ptr) - 1):
        toks = set(int(t) for t in q_terms[q_ptr[q]:q_ptr[q + 1]])
        out += [sum(len(lists.get((t, int(d)), ())) for t in toks) for d in hits["doc"][q, :n_hits[q]]]
    return out


@pytest.mark.parametrize("width", [1, 5, 20, 6000])
@pytest.mark.parametrize("k", [1, 10, 40])
def test_rows_of_score_topk_equal_the_model(ss_ctx, world, scorer, k, width):
    sc, ti, bi = scorer
    hits, n_hits, want = world_rows(world, sc, k, width)
    assert n_hits[3] == 0 and n_hits[2] == k
    got = passages(sc, world["q_ptr"], world["q_terms"], hits, n_hits, width)
    assert got.tobytes() == want
    assert got[3].tobytes() == bytes([FILL]) * (k * 24)                       # the query without hits: nothing is written
    assert (got["n_occ"][2, :k] > 0).any()
    if k == 40:
        n = raw_lengths(world, world["q_ptr"], world["q_terms"], hits, n_hits)
        # both sides of the caps test_small_cap_gives_the_same_bytes sets; the default cap of 512: test_a_doc_of_six_thousand_values
        assert min(n) <= 8 and sum(8 < x <= 64 for x in n) > 5 and sum(x > 64 for x in n) > 5 and max(n) <= 512


def test_device_chain_over_more_rounds_than_turns(ss_ctx, world, scorer):
    """score -> collapse -> explain -> passages, everything in device memory, four rounds back to back (more than the scorer has
    turns), alternating two batches, nothing waited for until the one synchronise at the end"""
    import torch
    sc, ti, bi = scorer
    lib = ss_ctx.lib
    k, g, width, t_stride = 10, 2, 20, 12
    group = (np.arange(world["n_docs"]) % 23).astype(np.uint32)
    sc.set_doc_groups(group)
    batches = [(world["q_ptr"], world["q_terms"]), queries([[3], [2, 1, 0], list(range(11, -1, -1))])]
    rounds = []
    for r in range(4):
        qp, qt = batches[r % 2]
        nq = len(qp) - 1
        rounds.append({"qp": qp, "qt": qt, "nq": nq,
                       "hits": torch.zeros(nq * k * 40, dtype=torch.uint8, device="cuda"), "n": torch.zeros(nq, dtype=torch.int32, device="cuda"),
                       "chits": torch.full((nq * k * 40,), FILL, dtype=torch.uint8, device="cuda"),
                       "cn": torch.zeros(nq, dtype=torch.int32, device="cuda"),
                       "exp": torch.full((nq * k * t_stride * 16,), FILL, dtype=torch.uint8, device="cuda"),
                       "pas": torch.full((nq * k * 24,), FILL, dtype=torch.uint8, device="cuda")})
    torch.cuda.synchronize()
    for c in rounds:
        qp, qt = c["qp"].ctypes.data, c["qt"].ctypes.data
        assert lib.ss_score_topk(sc.h, c["nq"], qp, qt, None, None, k, c["hits"].data_ptr(), c["n"].data_ptr()) == 0
        assert lib.ss_collapse_hits(sc.h, c["nq"], k, c["hits"].data_ptr(), c["n"].data_ptr(), g, 0, k, c["chits"].data_ptr(),
                                    c["cn"].data_ptr(), None, None) == 0
        assert lib.ss_explain_hits(sc.h, c["nq"], qp, qt, k, c["chits"].data_ptr(), c["cn"].data_ptr(), t_stride, c["exp"].data_ptr()) == 0
        assert lib.ss_best_passages(sc.h, c["nq"], qp, qt, k, c["chits"].data_ptr(), c["cn"].data_ptr(), width, c["pas"].data_ptr()) == 0
    ss_ctx.synchronize()
    for r, c in enumerate(rounds):
        rows, n_rows = sc.score_topk(c["qp"], c["qt"], k)
        crows, cn, _, _ = sc.collapse_hits(rows, n_rows, g, k)
        assert c["cn"].cpu().numpy().tolist() == cn.tolist() and int(cn.sum()) > 0
        got_rows = c["chits"].cpu().numpy().view(engine.HIT_DTYPE).reshape(c["nq"], k)
        assert all(got_rows[q, :cn[q]].tobytes() == crows[q, :cn[q]].tobytes() for q in range(c["nq"]))
        assert c["pas"].cpu().numpy().tobytes() == model(world, c["qp"], c["qt"], crows, cn, width).tobytes(), r
        exp = np.frombuffer(bytes([FILL]) * (c["nq"] * k * t_stride * 16), dtype=engine.TERM_MATCH_DTYPE).reshape(c["nq"], k, t_stride).copy()
        assert c["exp"].cpu().numpy().tobytes() == sc.explain_hits(c["qp"], c["qt"], crows, cn, t_stride=t_stride, out=exp).tobytes(), r
    # a device n_hits outside [0, k] is clamped by the kernel (host: refused, see the refusals test); mixed host / device arrays work
    hits, n_hits, _ = world_rows(world, sc, k, width)
    n_q = len(n_hits)
    d_bad = torch.tensor([k + 5, -3] + [0] * (n_q - 2), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    got = sc.best_passages(world["q_ptr"], world["q_terms"], hits, d_bad, width, out=prefilled(n_q, k))
    clamped = np.array([k, 0] + [0] * (n_q - 2), np.int32)
    assert got.tobytes() == model(world, world["q_ptr"], world["q_terms"], hits, clamped, width).tobytes()


def test_hand_cases_through_the_library(ss_ctx):
    n_docs, title, body, pos = hand_world()
    sc, ti, bi = make_scorer(ss_ctx, n_docs, title, body, np.ones(n_docs), np.ones(n_docs))
    try:
        def run(with_pos):
            for d, c in enumerate(HAND_CASES):
                q_ptr, q_terms = queries([c["tokens"]])
                hits, n_hits = made_up([[d]], k=2)
                got = passages(sc, q_ptr, q_terms, hits, n_hits, c["width"])
                want = pm.passages_ref(body, n_docs, q_ptr, q_terms, hits["doc"], n_hits, c["width"], body_pos=pos if with_pos else None, fill=FILL)
                assert got.tobytes() == want.tobytes(), c["name"]
                assert got[0, 1].tobytes() == bytes([FILL]) * 24
                e = got[0, 0]
                if with_pos:
                    assert np.array(c["want"][:2], np.float32).tobytes() == e["start"].tobytes() + e["last"].tobytes(), c["name"]
                    assert (int(e["n_distinct"]), int(e["n_occ"]), int(e["token_mask"])) == c["want"][2:], c["name"]
                else:
                    assert e.tobytes() == bytes(24)
        run(False)                                                            # no positions table: 24 zero bytes, written
        bi.set_positions(*pos)
        run(True)
        # made-up rows: docs at and past n_docs between real ones, slots behind n_hits naming a doc with a passage
        hits, n_hits = made_up([[0, n_docs, 1, UNKNOWN, 5], [7, 7], []], k=6)
        hits["doc"][:, 5] = 0
        hits["doc"][2, :] = 0
        q_ptr, q_terms = queries([[0, 1], [1, 0, 1], [0]])
        got = passages(sc, q_ptr, q_terms, hits, n_hits, 5)
        assert got.tobytes() == pm.passages_ref(body, n_docs, q_ptr, q_terms, hits["doc"], n_hits, 5, body_pos=pos, fill=FILL).tobytes()
        assert got[0, 1].tobytes() == bytes(24) and got[0, 3].tobytes() == bytes(24) and got["n_occ"][0, [0, 2, 4]].all()
        assert got[0, 5].tobytes() == bytes([FILL]) * 24 and got[2].tobytes() == bytes([FILL]) * (6 * 24)
        assert int(got["token_mask"][1, 0]) == 0b111
    finally:
        close_all(sc, ti, bi)


def test_small_cap_gives_the_same_bytes(ss_ctx, world, scorer):
    """"passage.lds_events" = 8 sends most hits of the batch down the global-memory path, 64 the hits with a long list; the default
    sends all of them through the LDS: both paths run on the same inputs and give the same bytes"""
    sc, ti, bi = scorer
    for k, width in ((40, 20), (10, 6000)):
        hits, n_hits, want = world_rows(world, sc, k, width)
        with ss_ctx.options(passage__lds_events=8):
            small = passages(sc, world["q_ptr"], world["q_terms"], hits, n_hits, width)
        with ss_ctx.options(passage__lds_events=64):
            mid = passages(sc, world["q_ptr"], world["q_terms"], hits, n_hits, width)
        dflt = passages(sc, world["q_ptr"], world["q_terms"], hits, n_hits, width)
        assert small.tobytes() == dflt.tobytes() == mid.tobytes() == want


def test_a_doc_of_six_thousand_values(ss_ctx):
    """one doc whose three terms hold 2,000 values each (more than any cap the option admits), beside a doc of 3 x 170 (just under the
    default cap of 512: the LDS sort at its full size) and one of 3 x 171 (just over)"""
    rng = np.random.default_rng(17)
    sizes = [2000, 170, 171]
    lists = []
    for t in range(3):
        for n in sizes:
            vals = rng.integers(0, 3000, size=n).astype(float)
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
        for width in (1, 20):
            got = passages(sc, q_ptr, q_terms, hits, n_hits, width)
            want = pm.passages_ref(body, 3, q_ptr, q_terms, hits["doc"], n_hits, width, body_pos=pos, fill=FILL)
            assert got.tobytes() == want.tobytes(), width
            assert got["n_distinct"][0, 0] == 3 and got["token_mask"][0, 0] == 0b1111 and (got["n_occ"][0] > 0).all()
    finally:
        close_all(sc, ti, bi)


def test_refusals_leave_out_untouched(ss_ctx, world, scorer):
    sc, ti, bi = scorer
    lib = ss_ctx.lib
    q_ptr, q_terms = queries([[0, 1, 2], [3]])
    hits, n_hits = sc.score_topk(q_ptr, q_terms, 4)
    out = prefilled(2, 4)

    def call(code, n_q=2, qp=q_ptr, qt=q_terms, k=4, h=hits, n=n_hits, width=20, o=out):
        ptr = lambda a: None if a is None else a.ctypes.data       # noqa: E731
        rc = lib.ss_best_passages(sc.h, n_q, ptr(qp), ptr(qt), k, ptr(h), ptr(n), width, ptr(o))
        assert rc == code, (rc, code)
        assert (out.view(np.uint8) == FILL).all()
    assert lib.ss_best_passages(None, 2, q_ptr.ctypes.data, q_terms.ctypes.data, 4, hits.ctypes.data, n_hits.ctypes.data, 20, out.ctypes.data) == ERR_INVALID
    assert (out.view(np.uint8) == FILL).all()
    call(ERR_INVALID, o=None)
    call(ERR_INVALID, n_q=-1)
    call(ERR_INVALID, k=0)
    call(ERR_INVALID, width=0)
    call(ERR_INVALID, width=-5)
    call(ERR_INVALID, qp=None)
    call(ERR_INVALID, qp=np.array([0, 3, 2], np.uint32))
    call(ERR_INVALID, qt=None)
    call(ERR_INVALID, h=None)
    call(ERR_INVALID, n=None)
    call(ERR_UNSUPPORTED, k=1025)
    call(ERR_UNSUPPORTED, width=(1 << 24) + 1)
    call(ERR_UNSUPPORTED, qp=np.array([0, 65, 66], np.uint32), qt=np.zeros(66, np.uint32))      # a query of 65 tokens
    call(ERR_UNSUPPORTED, n_q=1 << 21, k=1024, qp=np.zeros((1 << 21) + 1, np.uint32))           # 2^31 entries
    call(ERR_INVALID, n=np.array([5, 1], np.int32))
    call(ERR_INVALID, n=np.array([1, -1], np.int32))
    call(0, n_q=0)                                                      # nothing to do: SS_OK, nothing written
    with pytest.raises(SpaghettiError) as ei:
        sc.best_passages(q_ptr, q_terms, hits, n_hits, 0, out=out)
    assert ei.value.code == ERR_INVALID and (out.view(np.uint8) == FILL).all()
    # the largest width and a query of exactly 64 tokens are accepted, and the same arguments untouched
    q64 = queries([[t % 7 for t in range(64)], [3]])
    assert passages(sc, q64[0], q64[1], hits, n_hits, 1 << 24).tobytes() == model(world, q64[0], q64[1], hits, n_hits, 1 << 24).tobytes()
    assert passages(sc, q_ptr, q_terms, hits, n_hits, 20).tobytes() == model(world, q_ptr, q_terms, hits, n_hits, 20).tobytes()
