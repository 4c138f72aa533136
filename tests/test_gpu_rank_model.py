"""ss_rank_model_*, ss_hit_features and ss_rerank_hits_by_model on the GPU, byte for byte against the numpy model
(tests/rank_model_model.py), under "rank.lds_nodes" = default, 16 and 1: the LDS chunks, their padding-free seams and the walk from
global memory give the same bytes.  Rows are trusted by these calls, so most windows here are made up (docs, finals, NaN, -0.0) rather
than scored; the scorer is the golden 300 x 80 index, which gives n_docs and carries the field table."""
import numpy as np
import pytest

from spaghettisearch_amd import SpaghettiError, engine
from tests import rank_model_model as rm
from tests.test_gpu_score import close_all, make_scorer
from tests.test_passage_cpu import GOLDEN

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = 1, 7
FILL = 0xA5
CAPS = (None, 16, 1)
NF = rm.N_FEATURES
TILE = {15: 256, 64: 64}                                   # rows of one workgroup of k_forest_eval (header: 256 up to 16 features, else 64)


def prefilled(dtype, *shape):
    n = int(np.prod(shape))
    return np.frombuffer(bytes([FILL]) * (n * np.dtype(dtype).itemsize), dtype=dtype).reshape(shape).copy()


def untouched(*arrays):
    return all((a.view(np.uint8) == FILL).all() for a in arrays)


def under_caps(ss_ctx, call):
    """call() under every cap -> its results' bytes, after asserting that the three are the same"""
    got = []
    for cap in CAPS:
        with ss_ctx.options(rank__lds_nodes=cap):
            r = call()
        got.append(tuple(a.tobytes() for a in (r if isinstance(r, tuple) else (r,))))
    assert got[0] == got[1] == got[2]
    return got[0]


def device_model(ss_ctx, m):
    return engine.RankModel(ss_ctx, m["n_features"], m["trees"], linear=m["linear"], base=m["base"])


def check_eval(ss_ctx, m, x):
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, m["n_features"])
    dm = device_model(ss_ctx, m)
    try:
        got = under_caps(ss_ctx, lambda: dm.eval(x, out=prefilled(np.float64, len(x))))
        assert got[0] == rm.scores(m, x).tobytes()
        return dm.info()
    finally:
        dm.close()


def chain(n_splits, f=0):
    """a left-leaning chain: split i sends x <= i to the leaf i and everything else on; the last leaf is -1"""
    nodes = []
    for i in range(n_splits):
        nodes += [rm.split(f, float(i), 2 * i + 1, 2 * i + 2), rm.leaf(float(i))]
    return rm.tree(*nodes, rm.leaf(-1.0))


# ---- ss_rank_model_eval -----------------------------------------------------------------------------------------------------------------

def test_eval_small_models(ss_ctx):
    inf, nan = np.inf, np.nan
    rows3 = np.array([[0.5, -1.0, nan], [nan, 2.0, 0.0], [-0.0, 0.0, 1e300]])
    assert check_eval(ss_ctx, rm.model(3, [], None, 1.25), rows3) == {"n_features": 3, "n_trees": 0, "n_nodes": 0, "max_tree_nodes": 0, "max_depth": 0}
    check_eval(ss_ctx, rm.model(3, [], [2.0, 0.0, -0.5], -1.0), rows3)                 # linear alone; a NaN column and a zero weight are skipped
    check_eval(ss_ctx, rm.model(3, [], [1e300, 1e300, -1e300], 0.0), np.array([[5e9, -1e10, nan], [nan, 2e10, 0.0], [-0.0, 0.0, 1e10]]))   # +inf, -inf and inf - inf = the quiet NaN
    check_eval(ss_ctx, rm.model(3, [rm.tree(rm.leaf(7.5))]), rows3)                    # one tree that is a single leaf
    stump = lambda thr, nl=0: rm.tree(rm.split(0, thr, 1, 2, nl), rm.leaf(1.0), rm.leaf(2.0))   # noqa: E731
    edge = np.array([[0.5], [np.nextafter(0.5, 1)], [-0.0], [0.0], [inf], [-inf], [nan], [1e308]])
    for thr in (0.5, 0.0, -0.0, inf, -inf):                                            # x == value goes left; -0.0 <= +0.0; +-inf thresholds and values
        for nl in (0, 1):                                                              # a NaN feature under nan_left 0 and 1
            check_eval(ss_ctx, rm.model(1, [stump(thr, nl)]), edge)
    # sums where the order matters: 1e16 + 1.0 - 1e16 in tree order is 0.0, not 1.0 — under every chunking
    order = rm.model(2, [rm.tree(rm.leaf(1e16)), rm.tree(rm.leaf(1.0)), rm.tree(rm.leaf(-1e16))])
    check_eval(ss_ctx, order, [[0.0, 0.0]])
    assert rm.scores(order, [[0.0, 0.0]]).tolist() == [0.0]
    # the header's known answer
    m, x, want, _ = rm.known_answer()
    check_eval(ss_ctx, m, x)
    assert rm.scores(m, x).tobytes() == want.tobytes()


def test_eval_long_path_and_oversize_tree(ss_ctx):
    long = chain(70)                                                                   # a path longer than a wave
    x = np.array([[v] for v in (-5.0, 0.0, 0.5, 33.0, 68.5, 69.0, 69.5, np.nan, np.inf)])
    assert check_eval(ss_ctx, rm.model(1, [long]), x)["max_depth"] == 70
    # one tree above the default cap (1601 nodes > 1024) between two that fit; under cap 16 the 141-node chain is over it as well
    big = rm.model(2, [chain(3, 1), chain(800, 0), long, chain(2, 1)], [0.0, 0.25], 0.5)
    rng = np.random.default_rng(3)
    x = np.stack([rng.integers(-2, 810, 300).astype(np.float64), rng.integers(-1, 4, 300).astype(np.float64)], axis=1)
    x[::17, 0] = np.nan
    info = check_eval(ss_ctx, big, x)
    assert info["max_tree_nodes"] == 1601 and info["n_trees"] == 4


@pytest.mark.parametrize("nf", [15, 64])
def test_eval_random_forest_and_row_counts(ss_ctx, nf):
    rng = np.random.default_rng(nf)
    trees = [rm.random_tree(rng, 2 * int(rng.integers(0, 32)) + 1, nf) for _ in range(35)] + [rm.random_tree(rng, 1, nf), rm.random_tree(rng, 63, nf)]
    assert len(trees) == 37
    linear = np.where(rng.random(nf) < 0.5, 0.0, rng.normal(size=nf))
    m = rm.model(nf, trees, linear, 0.125)
    n_max = 2 * TILE[nf] + 1
    x = rm.random_rows(rng, n_max, nf)
    want = rm.scores(m, x)
    dm = device_model(ss_ctx, m)
    try:
        for n in (1, 63, 64, 65, TILE[nf], TILE[nf] + 1, n_max):
            out = prefilled(np.float64, n + 3)                                          # three entries behind the last row stay untouched
            got = under_caps(ss_ctx, lambda: dm.eval(x[:n], out=out))
            assert got[0][:8 * n] == want[:n].tobytes() and untouched(out[n:])
        assert dm.eval(np.zeros((0, nf))).shape == (0,)
    finally:
        dm.close()


def test_eval_device_tensors_and_refusals(ss_ctx):
    import torch
    m, x, want, _ = rm.known_answer()
    dm = device_model(ss_ctx, m)
    lib = ss_ctx.lib
    try:
        d_x, d_out = torch.from_numpy(x).cuda(), torch.from_numpy(prefilled(np.float64, 3)).cuda()
        torch.cuda.synchronize()
        for _ in range(4):                                                              # only enqueued
            assert lib.ss_rank_model_eval(dm.h, 3, d_x.data_ptr(), d_out.data_ptr()) == 0
        ss_ctx.synchronize()
        assert d_out.cpu().numpy().tobytes() == want.tobytes()
        assert dm.eval(d_x, out=prefilled(np.float64, 3)).tobytes() == want.tobytes()  # device in, host out
        out = prefilled(np.float64, 3)
        assert lib.ss_rank_model_eval(dm.h, -1, x.ctypes.data, out.ctypes.data) == ERR_INVALID
        assert lib.ss_rank_model_eval(dm.h, 1 << 31, x.ctypes.data, out.ctypes.data) == ERR_UNSUPPORTED
        assert lib.ss_rank_model_eval(dm.h, 3, None, out.ctypes.data) == ERR_INVALID
        assert lib.ss_rank_model_eval(dm.h, 3, x.ctypes.data, None) == ERR_INVALID
        assert lib.ss_rank_model_eval(None, 3, x.ctypes.data, out.ctypes.data) == ERR_INVALID
        assert lib.ss_rank_model_eval(dm.h, 0, None, None) == 0 and untouched(out)
        assert lib.ss_rank_model_get_info(dm.h, None) == ERR_INVALID and lib.ss_rank_model_get_info(None, out.ctypes.data) == ERR_INVALID
    finally:
        dm.close()
    assert lib.ss_rank_model_destroy(None) == ERR_INVALID


def test_create_refuses_invalid_models(ss_ctx):
    """every refusal of section 1 through the library (the same check_model the harness drives one case at a time): an invalid model
    never reaches the device, and the handle stays NULL"""
    import ctypes as C
    s, l = rm.split, rm.leaf
    lib = ss_ctx.lib

    def create(nf, trees, linear=None, base=0.0, tree_ptr=None, n_trees=None, null_nodes=False):
        ptr, nodes = rm.flat([np.asarray(t, dtype=rm.TREE_NODE) for t in trees])
        ptr = ptr if tree_ptr is None else np.array(tree_ptr, np.uint32)
        lin = None if linear is None else np.array(linear, np.float64)
        h = C.c_void_p()
        rc = lib.ss_rank_model_create(ss_ctx.h, nf, None if lin is None else lin.ctypes.data, base, len(ptr) - 1 if n_trees is None else n_trees,
                                      ptr.ctypes.data if len(ptr) else None, None if null_nodes or not len(nodes) else nodes.ctypes.data, C.byref(h))
        if rc == 0:
            assert h.value and lib.ss_rank_model_destroy(h) == 0
        else:
            assert not h.value
        return rc
    stump = [s(0, 0.5, 1, 2), l(1.0), l(2.0)]
    assert create(1, [stump]) == 0 and create(64, []) == 0 and create(1, [[s(0, np.inf, 1, 2), l(1.0), l(2.0)]]) == 0
    bad = [dict(nf=0, trees=[]), dict(nf=1, trees=[], n_trees=-1), dict(nf=1, trees=[], linear=[np.inf]), dict(nf=1, trees=[], base=np.nan),
           dict(nf=1, trees=[stump], tree_ptr=[1, 3]), dict(nf=1, trees=[stump, [l(0.0)]], tree_ptr=[0, 4, 3]),
           dict(nf=1, trees=[stump, [l(0.0)]], tree_ptr=[0, 3, 3, 4]), dict(nf=1, trees=[[s(1, 0.5, 1, 2), l(1.0), l(2.0)]]),
           dict(nf=1, trees=[[(-2, 0, 0, 0, 0.0)]]), dict(nf=1, trees=[[s(0, 0.5, 0, 2), l(1.0), l(2.0)]]), dict(nf=1, trees=[[s(0, 0.5, 1, 0), l(1.0), l(2.0)]]),
           dict(nf=1, trees=[[s(0, 0.5, 3, 2), l(1.0), l(2.0)]]), dict(nf=1, trees=[[s(0, 0.5, 1, 3), l(1.0), l(2.0)]]),
           dict(nf=1, trees=[[s(0, 0.5, 1, 2, 2), l(1.0), l(2.0)]]), dict(nf=1, trees=[[s(0, np.nan, 1, 2), l(1.0), l(2.0)]]),
           dict(nf=1, trees=[[s(0, 0.5, 1, 2), l(np.inf), l(2.0)]]), dict(nf=1, trees=[stump], null_nodes=True)]
    for case in bad:
        assert create(**case) == ERR_INVALID, case
    assert create(65, []) == ERR_UNSUPPORTED and create(1, [[l(0.0)]] * 8193) == ERR_UNSUPPORTED
    assert create(1, [[l(0.0)]], tree_ptr=[0, (1 << 24) + 1]) == ERR_UNSUPPORTED
    assert lib.ss_rank_model_create(ss_ctx.h, 1, None, 0.0, 0, None, None, None) == ERR_INVALID
    assert lib.ss_rank_model_create(None, 1, None, 0.0, 0, None, None, None) == ERR_INVALID
    with pytest.raises(SpaghettiError) as ei:
        engine.RankModel(ss_ctx, 1, [rm.tree(s(0, 0.5, 0, 2), l(1.0), l(2.0))])
    assert ei.value.code == ERR_INVALID


# ---- the window calls -------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def world():
    z = np.load(GOLDEN)
    n_docs = int(z["n_docs"])
    rng = np.random.default_rng(11)
    fields = rng.integers(-1000, 1000, size=(4, n_docs)).astype(np.int64)
    fields[0, 5], fields[1, 6], fields[3, 7] = rm.NO_FIELD_VALUE, (1 << 53) + 1, -(1 << 53) - 1     # absent; two values that round
    return {"n_docs": n_docs, "title": (z["t_ptr"], z["t_doc"], z["t_w"]), "body": (z["b_ptr"], z["b_doc"], z["b_w"]), "mt": z["t_mag"],
            "mb": z["b_mag"], "fields": fields}


@pytest.fixture()
def scorer(ss_ctx, world):
    sc, ti, bi = make_scorer(ss_ctx, world["n_docs"], world["title"], world["body"], world["mt"], world["mb"])
    yield sc
    close_all(sc, ti, bi)


def made_up_window(rng, n_docs, n_q, k_in, outside=0.05):
    """rows nobody scored: docs (some twice, some outside the table, 5 .. 7 among them), every double column random, a few NaN / -0.0"""
    hits = prefilled(engine.HIT_DTYPE, n_q, k_in)                                       # (_pad stays the fill: it is copied)
    hits["doc"] = rng.integers(0, n_docs, size=(n_q, k_in))
    hits["doc"][rng.random((n_q, k_in)) < outside] = n_docs + 3
    hits["doc"][:, :3] = [5, 6, 7][:min(3, k_in)]
    for name in ("title", "body", "pagerank", "final"):
        hits[name] = rng.choice([0.0, -0.0, 0.25, 0.5, 1.0, 2.0, np.nan, 1e300], size=(n_q, k_in), p=[.1, .1, .2, .2, .15, .15, .05, .05])
    prox = np.zeros((n_q, k_in), dtype=engine.PROXIMITY_DTYPE)
    prox["n_present"] = rng.integers(0, 5, size=(n_q, k_in))
    prox["start"] = rng.integers(0, 50, size=(n_q, k_in))
    prox["end"] = prox["start"] + rng.integers(0, 6, size=(n_q, k_in))
    prox["n_occ"] = rng.integers(0, 9, size=(n_q, k_in))
    prox["n_occ"][:, 0] = 0xFFFFFFFF
    vec = rng.integers(-(1 << 24), 1 << 24, size=(n_q, k_in)).astype(np.int32)
    vec[rng.random((n_q, k_in)) < 0.2] = rm.NO_VEC_SCORE
    qlen = rng.integers(1, 13, size=n_q).astype(np.int32)
    return hits, prox, vec, qlen


def test_hit_features(ss_ctx, world, scorer):
    import torch
    sc = scorer
    rng = np.random.default_rng(1)
    n_q, k_in, n_docs = 5, 70, world["n_docs"]
    hits, prox, vec, qlen = made_up_window(rng, n_docs, n_q, k_in)
    n_hits = np.array([k_in, 0, 1, 65, 37], np.int32)
    fill = prefilled(np.float64, n_q, k_in, NF)
    dev = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()   # noqa: E731
    for n_fields in (0, 2, 4):                                                          # 0: no table registered at all
        if n_fields:
            sc.set_doc_fields(world["fields"][:n_fields])
        fields = world["fields"][:n_fields] if n_fields else None
        for p, v, ql in ((None, None, None), (prox, None, None), (None, vec, None), (None, None, qlen), (prox, vec, qlen)):
            want = rm.features(hits, n_hits, n_docs, p, v, ql, fields, fill=fill)
            got = sc.hit_features(hits, n_hits, p, v, ql, out=fill.copy())
            assert got.tobytes() == want.tobytes(), (n_fields, p is not None, v is not None, ql is not None)
    want = rm.features(hits, n_hits, n_docs, prox, vec, qlen, world["fields"], fill=fill)
    assert want[0, 1, 12] == float(1 << 53) and want[0, 2, 14] == -float(1 << 53) and np.isnan(want[0, 0, 11])   # 2^53 + 1 rounds to even
    assert (want[0, 0, 0:4].view(np.uint64) == hits[0, 0:1].view(np.uint64)[1:5]).all()                         # the rows' bytes as given
    # everything on the device, only enqueued; then mixed host / device optional arrays
    d_hits, d_n, d_out = dev(hits), torch.from_numpy(n_hits.copy()).cuda(), torch.from_numpy(fill.copy()).cuda()
    d_prox, d_vec, d_qlen = dev(prox), torch.from_numpy(vec.copy()).cuda(), torch.from_numpy(qlen.copy()).cuda()
    torch.cuda.synchronize()
    for _ in range(4):
        assert ss_ctx.lib.ss_hit_features(sc.h, n_q, k_in, d_hits.data_ptr(), d_n.data_ptr(), d_prox.data_ptr(), d_vec.data_ptr(), d_qlen.data_ptr(),
                                          d_out.data_ptr()) == 0
    ss_ctx.synchronize()
    assert d_out.cpu().numpy().tobytes() == want.tobytes()
    assert sc.hit_features(d_hits, n_hits, prox, d_vec, qlen, k_in=k_in, out=fill.copy()).tobytes() == want.tobytes()
    assert sc.hit_features(hits, d_n, d_prox, vec, d_qlen, out=fill.copy()).tobytes() == want.tobytes()
    # a device n_hits outside [0, k_in] is clamped (host: refused)
    d_bad = torch.tensor([k_in + 9, -4, 1, 0, 2], dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    got = sc.hit_features(hits, d_bad, prox, vec, qlen, out=fill.copy())
    assert got.tobytes() == rm.features(hits, np.array([k_in, 0, 1, 0, 2]), n_docs, prox, vec, qlen, world["fields"], fill=fill).tobytes()
    # refusals, the output untouched
    lib, out = ss_ctx.lib, fill.copy()
    ptr = lambda a: None if a is None else a.ctypes.data       # noqa: E731

    def refused(code, n_q=n_q, k_in=k_in, h=hits, n=n_hits, o=out):
        assert lib.ss_hit_features(sc.h, n_q, k_in, ptr(h), ptr(n), ptr(prox), ptr(vec), ptr(qlen), ptr(o)) == code
        assert untouched(out)
    assert lib.ss_hit_features(None, n_q, k_in, ptr(hits), ptr(n_hits), None, None, None, ptr(out)) == ERR_INVALID
    refused(ERR_INVALID, n_q=-1)
    refused(ERR_INVALID, k_in=0)
    refused(ERR_UNSUPPORTED, k_in=1025)
    refused(ERR_UNSUPPORTED, n_q=1 << 21, k_in=1024)
    refused(ERR_INVALID, h=None)
    refused(ERR_INVALID, n=None)
    refused(ERR_INVALID, o=None)
    refused(ERR_INVALID, n=np.array([k_in + 1, 0, 0, 0, 0], np.int32))
    refused(ERR_INVALID, n=np.array([0, 0, -1, 0, 0], np.int32))
    refused(0, n_q=0)


def window_model(nf_trees=5, seed=7):
    rng = np.random.default_rng(seed)
    trees = [rm.random_tree(rng, 2 * int(rng.integers(1, 16)) + 1, NF) for _ in range(nf_trees)]
    # thresholds that the columns' values meet: positions, counts and field values are not in rm.VALUES
    for t in trees:
        for nd in t:
            if nd["feature"] in (4, 5, 6, 7, 9):
                nd["value"] = float(rng.integers(0, 12))
            elif nd["feature"] >= 10:
                nd["value"] = float(rng.integers(-500, 500))
    linear = np.zeros(NF)
    linear[[3, 8, 10]] = [1.0, 0.5, 1e-7]
    return rm.model(NF, trees, linear, 0.0)


def rerank_out(n_q, k):
    return prefilled(engine.HIT_DTYPE, n_q, k), prefilled(np.int32, n_q), prefilled(np.float64, n_q, k)


def model_rerank(m, world, hits, n_hits, first, k, prox=None, vec=None, qlen=None):
    n_q = hits.shape[0]
    o = rerank_out(n_q, k)
    return rm.rerank(m, hits, n_hits, world["n_docs"], first, k, prox, vec, qlen, world["fields"], hits_fill=o[0], scores_fill=o[2])


@pytest.mark.parametrize("k_in", [1, 2, 100, 1024])
def test_rerank_windows(ss_ctx, world, scorer, k_in):
    sc = scorer
    sc.set_doc_fields(world["fields"])
    rng = np.random.default_rng(k_in)
    n_q = 3
    hits, prox, vec, qlen = made_up_window(rng, world["n_docs"], n_q, k_in, outside=0.1)
    hits["final"][0, : k_in // 2] = 0.5                                                 # equal scores under the linear model below: stable
    n_hits = np.array([k_in, k_in - k_in // 3, min(k_in, 1)], np.int32)
    m = window_model()
    tie = rm.model(NF, [], np.eye(NF)[3], 0.0)                                          # score = final: ties, NaN finals, -0.0 against 0.0
    dm, dt = device_model(ss_ctx, m), device_model(ss_ctx, tie)
    try:
        for first, k in ((0, min(k_in, 10)), (k_in // 2, 7), (k_in - 1, 3), (k_in, 2), (k_in + 5, 2), (0, k_in)):   # inside, at and past the end
            want = model_rerank(m, world, hits, n_hits, first, k, prox, vec, qlen)
            got = under_caps(ss_ctx, lambda: sc.rerank_by_model(dm, hits, n_hits, k, prox, vec, qlen, first, out=rerank_out(n_q, k)))
            assert got == tuple(a.tobytes() for a in want), (first, k)
        k = min(k_in, 40)
        want = model_rerank(tie, world, hits, n_hits, 0, k)
        got = sc.rerank_by_model(dt, hits, n_hits, k, out=rerank_out(n_q, k))
        assert tuple(a.tobytes() for a in got) == tuple(a.tobytes() for a in want)
        o = rerank_out(n_q, k)
        bare = sc.rerank_by_model(dt, hits, n_hits, k, out=(o[0], o[1], None), want_scores=False)      # scores_out NULL
        assert (bare[0].tobytes(), bare[1].tobytes()) == (want[0].tobytes(), want[1].tobytes()) and bare[2] is None
        if k_in >= 100:                                                                # the window has every class: numbers, NaN scores, outside rows
            inside = hits["doc"][0] < world["n_docs"]
            assert np.isnan(hits["final"][0][inside]).any() and not inside.all() and len(set(hits["doc"][0][inside].tolist())) < inside.sum()
    finally:
        dm.close()
        dt.close()


def test_rerank_identity_known_answer_and_devices(ss_ctx, world, scorer):
    import torch
    sc = scorer
    sc.set_doc_fields(world["fields"])
    z = np.load(GOLDEN)
    q_ptr, q_terms = np.array([0, 3, 4, 6], np.uint32), np.array([0, 1, 2, 3, 70, 5], np.uint32)
    k_in, first, k = 40, 0, 10
    hits, n_hits = sc.score_topk(q_ptr, q_terms, k_in)
    assert not np.isnan(hits["final"]).any() and (n_hits > k).all() and int(z["n_docs"]) == world["n_docs"]
    n_q = len(n_hits)
    # linear[3] = 1 and nothing else on a window in FinalRank order: the page is the window's page (the family's w_prox == 0 identity)
    ident = device_model(ss_ctx, rm.model(NF, [], np.eye(NF)[3], 0.0))
    m = window_model(seed=9)
    dm = device_model(ss_ctx, m)
    try:
        for first in (0, 5):
            o_hits, o_n, o_sc = sc.rerank_by_model(ident, hits, n_hits, k, first=first, out=rerank_out(n_q, k))
            assert o_hits.tobytes() == hits[:, first:first + k].tobytes() and o_n.tolist() == [k] * n_q
            assert o_sc.tobytes() == hits["final"][:, first:first + k].tobytes()
        # the header's known answer as a window: no prox array (absent: NaN goes right), field 0 from a table of its own
        ka, _, _, _ = rm.known_answer()
        dka = device_model(ss_ctx, ka)
        try:
            w = np.zeros((1, 3), dtype=engine.HIT_DTYPE)
            w["doc"], w["final"] = [[0, 1, 2]], [[1.0, 1.5, 1.0]]
            f0 = np.zeros((1, world["n_docs"]), np.int64)
            f0[0, :3] = [50, rm.NO_FIELD_VALUE, 200]
            sc.set_doc_fields(f0)
            o_hits, o_n, o_sc = sc.rerank_by_model(dka, w, np.array([3], np.int32), 3)
            assert o_hits["doc"].tolist() == [[1, 0, 2]] and o_sc.tolist() == [[4.75, 3.75, 3.25]]
        finally:
            dka.close()
            sc.set_doc_fields(world["fields"])
        # scored rows with the real proximity entries and vector-free features: host arrays, then everything on the device with no wait
        first = 3
        prox = np.zeros((n_q, k_in), dtype=engine.PROXIMITY_DTYPE)                      # (the golden body table has no positions: zero entries)
        qlen = np.array([3, 1, 2], np.int32)
        want = tuple(a.tobytes() for a in model_rerank(m, world, hits, n_hits, first, k, prox, None, qlen))
        got = sc.rerank_by_model(dm, hits, n_hits, k, prox, None, qlen, first, out=rerank_out(n_q, k))
        assert tuple(a.tobytes() for a in got) == want
        dev = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()   # noqa: E731
        filled = lambda n: torch.full((n,), FILL, dtype=torch.uint8, device="cuda")   # noqa: E731
        d_hits, d_n, d_prox, d_qlen = dev(hits), torch.from_numpy(n_hits.copy()).cuda(), dev(prox), torch.from_numpy(qlen).cuda()
        d_o = (filled(n_q * k * 40), torch.full((n_q,), -1, dtype=torch.int32, device="cuda"), torch.from_numpy(prefilled(np.float64, n_q, k)).cuda())
        torch.cuda.synchronize()
        for _ in range(4):                                                             # more rounds than the scorer has turns, nothing waited for
            assert ss_ctx.lib.ss_rerank_hits_by_model(sc.h, dm.h, n_q, k_in, d_hits.data_ptr(), d_n.data_ptr(), d_prox.data_ptr(), None, d_qlen.data_ptr(),
                                                      first, k, *(t.data_ptr() for t in d_o)) == 0
        ss_ctx.synchronize()
        assert tuple(t.cpu().numpy().tobytes() for t in d_o) == want
        o = rerank_out(n_q, k)
        mixed = sc.rerank_by_model(dm, d_hits, n_hits, k, d_prox, None, qlen, first, k_in=k_in, out=(filled(n_q * k * 40), o[1], o[2]))
        assert (mixed[0].cpu().numpy().tobytes(), mixed[1].tobytes(), mixed[2].tobytes()) == want
        d_bad = torch.tensor([k_in + 5, -3, 2], dtype=torch.int32, device="cuda")      # clamped by the kernels
        torch.cuda.synchronize()
        got = sc.rerank_by_model(dm, hits, d_bad, k, prox, None, qlen, first, out=rerank_out(n_q, k))
        assert tuple(a.tobytes() for a in got) == tuple(a.tobytes() for a in model_rerank(m, world, hits, np.array([k_in, 0, 2]), first, k, prox, None, qlen))
    finally:
        ident.close()
        dm.close()


def test_rerank_refusals_leave_the_outputs_untouched(ss_ctx, world, scorer):
    sc = scorer
    lib = ss_ctx.lib
    rng = np.random.default_rng(4)
    hits, prox, vec, qlen = made_up_window(rng, world["n_docs"], 2, 4)
    n_hits = np.array([4, 2], np.int32)
    o = rerank_out(2, 3)
    ptr = lambda a: None if a is None else a.ctypes.data       # noqa: E731
    good = device_model(ss_ctx, window_model())
    narrow = device_model(ss_ctx, rm.model(14, []))
    wide = device_model(ss_ctx, rm.model(16, []))
    other_ctx = engine.Context(0)
    foreign = device_model(other_ctx, window_model())
    try:
        def paged(code, model=good, n_q=2, k_in=4, h=hits, n=n_hits, first=0, k=3, oh=o[0], on=o[1], osc=o[2]):
            rc = lib.ss_rerank_hits_by_model(sc.h, model.h if model else None, n_q, k_in, ptr(h), ptr(n), ptr(prox), ptr(vec), ptr(qlen), first, k,
                                             ptr(oh), ptr(on), ptr(osc))
            assert rc == code, (rc, code)
            assert untouched(*o)
        assert lib.ss_rerank_hits_by_model(None, good.h, 2, 4, ptr(hits), ptr(n_hits), None, None, None, 0, 3, *(ptr(a) for a in o)) == ERR_INVALID
        paged(ERR_INVALID, model=None)
        paged(ERR_INVALID, model=narrow)                                                # n_features != SS_RANK_N_FEATURES
        paged(ERR_INVALID, model=wide)
        paged(ERR_INVALID, model=foreign)                                               # a model of another context
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
        paged(ERR_INVALID, n=np.array([5, 1], np.int32))
        paged(ERR_INVALID, n=np.array([1, -1], np.int32))
        both = prefilled(engine.HIT_DTYPE, 2, 8)
        rc = lib.ss_rerank_hits_by_model(sc.h, good.h, 2, 4, both.ctypes.data, ptr(n_hits), None, None, None, 0, 3, both.ctypes.data + 7 * 40, ptr(o[1]), None)
        assert rc == ERR_INVALID and untouched(both, *o)                                # hits_out overlaps hits
        paged(0, n_q=0)
        with pytest.raises(SpaghettiError) as ei:
            sc.rerank_by_model(narrow, hits, n_hits, 3, out=o)
        assert ei.value.code == ERR_INVALID and untouched(*o)
    finally:
        for d in (good, narrow, wide, foreign):
            d.close()
        other_ctx.close()
