"""GPU parity: doc fields (ss_scorer_set_doc_fields, ss_doc_field_masks, ss_score_topk_filtered, ss_sort_hits_by_field, ss_hit_fields)
vs the model of the header's definitions (tests/doc_fields_model.py) and vs ss_score_topk_masked over the model's sets.  Every
comparison is bit-exact: tobytes() on whole output arrays that start from 0xA5 bytes, so an entry a call must not write is checked
with the ones it must."""
import numpy as np
import pytest

from spaghettisearch_amd import SpaghettiError, engine
from tests import doc_fields_model as fm
from tests.test_gpu_collapse import FILL, as_bytes, filled, random_rows
from tests.test_gpu_query_constraints import Contains, allowed_sets, pack_pairs
from tests.test_gpu_score import build_weighted, close_all, make_scorer

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE, ERR_UNSUPPORTED = 1, 6, 7
B = 8192                         # docs of one k_field_masks workgroup: FM_DOCS in csrc/field.hip (test_doc_fields_cpu.py reads it there)
G = 64                           # sets that share one read of the columns: FM_GROUP
I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1
UNKNOWN = 0xFFFFFFFF
TINY = (np.array([0, 1], np.uint64), np.array([0], np.uint32), np.array([1.0], np.float32))      # one posting: the tables do not matter


def tiny_scorer(ss_ctx, n_docs):
    return make_scorer(ss_ctx, n_docs, TINY, TINY, np.ones(n_docs), np.ones(n_docs))


def field_table(rng, n_docs):
    """four columns: a date-like uniform one, a size-like skewed one, one of extreme values, one constant"""
    edge = np.array([I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX - 1, I64_MAX], np.int64)
    return np.stack([rng.integers(0, 1000, n_docs), (rng.lognormal(9.0, 1.5, n_docs)).astype(np.int64) - 5000,
                     edge[rng.integers(0, len(edge), n_docs)], np.full(n_docs, 7)]).astype(np.int64)


def random_sets(rng, n_sets, n_fields):
    """0, 1, 2 or 4 clauses a set on 1 to n_fields fields: about half / a twentieth of the docs, everything, nothing, lo == hi,
    lo > hi, the extremes"""
    def clause():
        f = int(rng.integers(0, n_fields))
        c = rng.random()
        if f == 0:
            lo = int(rng.integers(0, 500))
            return (f, lo, lo + (500 if c < 0.6 else 50 if c < 0.9 else 0))
        if f == 1:
            return (f, I64_MIN, 3000) if c < 0.5 else (f, 3000, I64_MAX) if c < 0.8 else (f, 100000, 50000)
        if f == 2:
            pick = [(I64_MIN, I64_MIN), (I64_MIN, -1), (0, I64_MAX), (I64_MAX, I64_MAX), (-1, 1), (I64_MIN, I64_MAX), (1, -1)]
            return (f,) + pick[int(rng.integers(0, len(pick)))]
        return (f, 7, 7) if c < 0.7 else (f, 8, I64_MAX)
    return [[clause() for _ in range(int(rng.choice([0, 1, 1, 2, 2, 4])))] for _ in range(n_sets)]


# ---- ss_doc_field_masks ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_docs", [1, 31, 32, 33, 63, 64, 65, B - 1, B, B + 1, 2 * B + 37])
def test_field_masks_sizes(ss_ctx, n_docs):
    """every table size around a word, a wave step and a workgroup's seam; set counts of 1, one group, one group + 1 and three
    groups + 1; 1 to 4 fields; a registered base mask and -1; a set with no clause; duplicate sets; host and device outputs"""
    import torch
    rng = np.random.default_rng(n_docs)
    sc, ti, bi = tiny_scorer(ss_ctx, n_docs)
    try:
        masks = rng.random((3, n_docs)) < np.array([0.5, 0.05, 1.0])[:, None]
        sc.set_doc_masks(engine.pack_doc_masks(masks, n_docs))
        for n_fields, n_sets in ((1, 1), (2, G), (3, G + 1), (4, 3 * G + 1)):
            values = field_table(rng, n_docs)[:n_fields]
            sc.set_doc_fields(values)
            sets = random_sets(rng, n_sets, n_fields)
            sets[0] = [] if n_sets > 1 else [(0, 0, 499)]
            if n_sets > 2:
                sets[-1] = sets[1]                                            # a duplicate, in another group when there is one
            for mask_id in (None, rng.integers(-1, 3, n_sets).astype(np.int32)):
                want = fm.set_words(values, n_docs, sets, mask_id, masks)
                got = sc.doc_field_masks(engine.pack_doc_ranges(sets), mask_id, out=filled(want.shape, np.uint32))
                assert got.tobytes() == want.tobytes(), (n_fields, n_sets, mask_id is None)
                d_out = torch.full((want.size,), -1, dtype=torch.int32, device="cuda")
                sc.doc_field_masks(engine.pack_doc_ranges(sets), mask_id, out=d_out)
                ss_ctx.synchronize()
                assert d_out.cpu().numpy().tobytes() == want.tobytes(), (n_fields, n_sets)
        # the last word's dead bits stay 0 where everything matches, and the output registers as it is
        everything = sc.doc_field_masks(engine.pack_doc_ranges([[], [(0, I64_MIN, I64_MAX)]]))
        assert everything.tobytes() == engine.pack_doc_masks(np.ones((2, n_docs), bool), n_docs).tobytes()
        sc.set_doc_masks(everything)
    finally:
        close_all(sc, ti, bi)


# ---- ss_score_topk_filtered -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def world(oracle):
    n_docs, n_terms = 2 * B + 3000, 600
    title, body, mt, mb = build_weighted(oracle, n_docs, n_terms, 300000, 30000, seed=77)
    rng = np.random.default_rng(78)
    return {"n_docs": n_docs, "n_terms": n_terms, "title": title, "body": body, "mt": mt, "mb": mb, "values": field_table(rng, n_docs),
            "masks": rng.random((2, n_docs)) < np.array([0.5, 0.1])[:, None]}


@pytest.fixture()
def scorer(ss_ctx, world):
    sc, ti, bi = make_scorer(ss_ctx, world["n_docs"], world["title"], world["body"], world["mt"], world["mb"])
    sc.set_doc_fields(world["values"])
    yield sc, ti, bi
    close_all(sc, ti, bi)


def queries(rng, n_q, n_terms):
    lens = rng.integers(1, 5, size=n_q)
    q_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    return q_ptr, np.minimum(rng.geometric(0.02, size=int(lens.sum())) - 1, n_terms + 2).astype(np.uint32)


def check_filtered(sc, world, q_ptr, q_terms, clauses, k, req=None, exc=None, mask_id=None, **kw):
    """the filtered call equals ss_score_topk_masked over the model's sets, one registered per query; leaves world's masks registered"""
    n_docs, n_q = world["n_docs"], len(q_ptr) - 1
    req = req or [[] for _ in range(n_q)]
    exc = exc or [[] for _ in range(n_q)]
    hits, n_hits = sc.score_topk_filtered(q_ptr, q_terms, k, ranges=engine.pack_doc_ranges(clauses), req=pack_pairs(req),
                                          exc=pack_pairs(exc), mask_id=mask_id, **kw)
    ids, sets = allowed_sets(Contains(n_docs, world["title"], world["body"]), n_docs, req, exc, mask_id, world["masks"])
    per_q = np.ones((n_q, n_docs), dtype=bool)
    for q in range(n_q):
        if ids[q] >= 0:
            per_q[q] = sets[ids[q]]
        per_q[q] &= fm.matches(world["values"], n_docs, clauses[q])
    sc.set_doc_masks(engine.pack_doc_masks(per_q, n_docs))
    ref, ref_n = sc.score_topk_masked(q_ptr, q_terms, np.arange(n_q, dtype=np.int32), k, **kw)
    sc.set_doc_masks(engine.pack_doc_masks(world["masks"], n_docs))
    assert n_hits.tolist() == ref_n.tolist()
    assert hits.tobytes() == ref.tobytes()
    return hits, n_hits


@pytest.mark.parametrize("small", [0, 1], ids=["small-kernel-off", "small-kernel-on"])
def test_filtered_random_batch(ss_ctx, world, scorer, small):
    """ranges alone, with a mask, with + / - terms; queries sharing a clause set and queries with their own; clauses that allow
    nothing and everything.  Not vacuous: at least half of the queries return a non-empty row that differs from the unfiltered one."""
    sc = scorer[0]
    ss_ctx.set_option("score.small", small)
    try:
        rng = np.random.default_rng(5)
        n_q, k = 96, 20
        q_ptr, q_terms = queries(rng, n_q, world["n_terms"])
        shared = [[(0, 0, 499)], [(0, 100, 149)], [(0, 0, 499), (1, I64_MIN, 3000)], [(2, 1, -1)], [(2, I64_MIN, I64_MAX)], []]
        # a query's own window of dates, about 50 % or 5 % of the docs, half of them with a size clause too
        own = [[(0, lo, lo + (499 if q % 4 else 49))] + ([(1, I64_MIN, 3000)] if q % 8 == 0 else [])
               for q, lo in enumerate(rng.integers(0, 500, n_q).tolist())]
        clauses = [shared[(q // 2) % len(shared)] if q % 2 else own[q] for q in range(n_q)]
        sc.set_doc_masks(engine.pack_doc_masks(world["masks"], world["n_docs"]))
        plain, plain_n = sc.score_topk(q_ptr, q_terms, k)
        hits, n_hits = check_filtered(sc, world, q_ptr, q_terms, clauses, k)
        differs = sum(1 for q in range(n_q) if n_hits[q] > 0 and hits[q, :n_hits[q]].tobytes() != plain[q, :plain_n[q]].tobytes())
        assert 2 * differs >= n_q, differs
        assert (n_hits == 0).any() and any(hits[q].tobytes() == plain[q].tobytes() and plain_n[q] > 0 for q in range(n_q))
        mask_id = rng.integers(-1, 2, n_q).astype(np.int32)
        check_filtered(sc, world, q_ptr, q_terms, clauses, k, mask_id=mask_id)
        req = [[int(rng.integers(0, 30))] if rng.random() < 0.4 else [] for _ in range(n_q)]
        exc = [[int(rng.integers(0, 30)), UNKNOWN] if rng.random() < 0.4 else [] for _ in range(n_q)]
        check_filtered(sc, world, q_ptr, q_terms, clauses, 300, req=req, exc=exc, mask_id=mask_id)
        # the clauses of a query as a set: order and repeats change nothing
        twice = [c[::-1] + c[:1] if 0 < len(c) < 4 else c for c in clauses]
        again, again_n = sc.score_topk_filtered(q_ptr, q_terms, k, ranges=engine.pack_doc_ranges(twice))
        assert again.tobytes() == hits.tobytes() and again_n.tolist() == n_hits.tolist()
    finally:
        ss_ctx.set_option("score.small", None)


def test_filtered_topic_priors(world, scorer):
    sc = scorer[0]
    rng = np.random.default_rng(6)
    n_q = 40
    q_ptr, q_terms = queries(rng, n_q, world["n_terms"])
    sc.set_prior(rng.random((4, world["n_docs"])) * 1e-3)
    probs = rng.dirichlet(np.ones(4), size=n_q)
    check_filtered(sc, world, q_ptr, q_terms, random_sets(rng, n_q, 4), 30, topic_probs=probs)


def test_filtered_phrases(ss_ctx, oracle):
    from tests.test_gpu_phrase import positional_table
    n_docs, n_terms = 3000, 40
    (bt, bpos) = positional_table(n_docs, n_terms, 30000, seed=15)
    (tt, tpos) = positional_table(n_docs, n_terms, 4000, seed=16, max_pos=8, anchor_frac=0.5)
    wb, mb, _ = oracle.tfidf(*bt, n_docs, n_docs)
    wt, mt, _ = oracle.tfidf(*tt, n_docs, n_docs)
    w = {"n_docs": n_docs, "title": (tt[0], tt[1], wt), "body": (bt[0], bt[1], wb), "masks": np.ones((1, n_docs), bool),
         "values": field_table(np.random.default_rng(3), n_docs)}
    sc, ti, bi = make_scorer(ss_ctx, n_docs, w["title"], w["body"], mt, mb)
    try:
        ti.set_positions(*tpos)
        bi.set_positions(*bpos)
        sc.set_doc_fields(w["values"])
        q_ptr, q_terms = pack_pairs([[0, 3], [], [5], [2, 2], [4], [7, 1]])
        p_ptr, p_terms = pack_pairs([[1, 2], [0, 1], [2, 0], [1, 1], [0, 99], []])
        clauses = [[(0, 0, 499)], [(0, 0, 499)], [(1, I64_MIN, 3000), (0, 250, 999)], [], [(0, 0, 999)], [(0, 100, 149)]]
        hits, n_hits = check_filtered(sc, w, q_ptr, q_terms, clauses, 50, p_ptr=p_ptr, p_terms=p_terms)
        assert n_hits[[0, 2, 3]].min() > 0
    finally:
        close_all(sc, ti, bi)


def test_no_clause_is_the_constrained_call(world, scorer):
    sc = scorer[0]
    rng = np.random.default_rng(7)
    n_q, k = 48, 25
    q_ptr, q_terms = queries(rng, n_q, world["n_terms"])
    sc.set_doc_masks(engine.pack_doc_masks(world["masks"], world["n_docs"]))
    mask_id = rng.integers(-1, 2, n_q).astype(np.int32)
    req = pack_pairs([[int(rng.integers(0, 30))] if q % 3 == 0 else [] for q in range(n_q)])
    exc = pack_pairs([[int(rng.integers(0, 30))] if q % 4 == 0 else [] for q in range(n_q)])
    want = sc.score_topk_constrained(q_ptr, q_terms, k, req=req, exc=exc, mask_id=mask_id)
    none = (np.zeros(n_q + 1, np.uint32), np.zeros(0, engine.DOC_RANGE_DTYPE))
    for ranges in (None, none):
        got = sc.score_topk_filtered(q_ptr, q_terms, k, ranges=ranges, req=req, exc=exc, mask_id=mask_id)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tolist() == want[1].tolist()
    sc.set_doc_fields(None)                                                   # ... and needs no field table
    got = sc.score_topk_filtered(q_ptr, q_terms, k, ranges=none, req=req, exc=exc, mask_id=mask_id)
    assert got[0].tobytes() == want[0].tobytes()


# ---- ss_sort_hits_by_field, ss_hit_fields -------------------------------------------------------------------------------------------

def sort_outputs(n_q, k):
    return filled((n_q, k), engine.HIT_DTYPE), filled(n_q, np.int32), filled((n_q, k), np.int64)


def check_sort(sc, hits, n_hits, values, n_docs, field, desc, first, k, tag=None):
    want = fm.sort_page(hits, n_hits, values, n_docs, field, desc, first, k, *sort_outputs(hits.shape[0], k))
    got = sc.sort_hits_by_field(hits, n_hits, field, k, descending=desc, first=first, out=sort_outputs(hits.shape[0], k))
    assert as_bytes(got) == as_bytes(want), (tag, field, desc, first, k)
    return got


def check_gather(ss_ctx, sc, hits, n_hits, values, n_docs, tag=None):
    """ss_hit_fields against the model: host arrays; device arrays; device counts out of range, clamped by the kernel"""
    import torch
    n_q, k_in = hits.shape
    shape = (n_q, k_in, len(values))
    want = fm.gather(hits, n_hits, values, n_docs, filled(shape, np.int64))
    got = sc.hit_fields(hits, n_hits, out=filled(shape, np.int64))
    assert got.tobytes() == want.tobytes(), (tag, "host")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()      # noqa: E731
    bad = n_hits.copy()
    bad[0], bad[-1] = -3, k_in + 9
    for counts, ref in ((n_hits, want), (bad, fm.gather(hits, bad, values, n_docs, filled(shape, np.int64), clamp=True))):
        d_out = dev(filled(shape, np.int64))
        torch.cuda.synchronize()
        assert ss_ctx.lib.ss_hit_fields(sc.h, n_q, k_in, dev(hits).data_ptr(), dev(counts).data_ptr(), d_out.data_ptr()) == 0
        ss_ctx.synchronize()
        assert d_out.cpu().numpy().tobytes() == ref.tobytes(), (tag, "device", counts is bad)
    return got


@pytest.mark.parametrize("k_in", [1, 2, 63, 64, 65, 1024])
def test_sort_window_sizes(ss_ctx, k_in):
    n_docs = 1100
    sc, ti, bi = tiny_scorer(ss_ctx, n_docs)
    try:
        rng = np.random.default_rng(k_in)
        values = np.stack([rng.integers(0, 5, n_docs), rng.permutation(n_docs) - 500, np.full(n_docs, -3),
                           np.array([I64_MIN, -1, 0, I64_MAX])[rng.integers(0, 4, n_docs)]]).astype(np.int64)
        sc.set_doc_fields(values)
        lengths = sorted({0, 1, k_in // 2, k_in - 1, k_in})
        n_hits = np.array(lengths, np.int32)
        hits = random_rows(rng, len(lengths), k_in, n_docs + 40)              # docs n_docs .. n_docs + 39: outside the table; docs repeat
        hits["doc"][0, :1] = UNKNOWN
        hits["doc"][-1, -1] = UNKNOWN                                         # (the full window: a row outside the table at its end ...
        hits["doc"][-1, :2] = 5                                               #  ... and the same doc twice; at k_in = 1 doc 5 alone)
        for field in range(4):                                                # ties, all distinct, all equal, the extremes
            for desc in (False, True):
                for first, k in ((0, k_in), (0, 1024), (k_in // 2, 7), (max(k_in - 1, 0), 3), (k_in, 3), (k_in + 1, 3), (2 ** 31 - 1, 1)):
                    check_sort(sc, hits, n_hits, values, n_docs, field, desc, first, k, k_in)
        got = sc.sort_hits_by_field(hits, n_hits, 1, k_in, want_values=False)    # values_out NULL
        want = fm.sort_page(hits, n_hits, values, n_docs, 1, False, 0, k_in, np.zeros_like(got[0]), np.zeros_like(got[1]))
        assert got[2] is None and got[0].tobytes() == want[0].tobytes() and got[1].tolist() == want[1].tolist()
        # ss_hit_fields on the same windows: four fields, then three and one (the entry index is divided by the field count)
        for n_fields in (4, 3, 1):
            sc.set_doc_fields(values[:n_fields])
            check_gather(ss_ctx, sc, hits, n_hits, values[:n_fields], n_docs, (k_in, n_fields))
    finally:
        close_all(sc, ti, bi)


def test_hit_fields_and_pointer_placements(ss_ctx):
    import torch
    n_docs, n_q, k_in, k, first = 700, 7, 130, 40, 3
    sc, ti, bi = tiny_scorer(ss_ctx, n_docs)
    try:
        lib = ss_ctx.lib
        rng = np.random.default_rng(12)
        values = field_table(rng, n_docs)[:3]
        sc.set_doc_fields(values)
        hits = random_rows(rng, n_q, k_in, n_docs + 9)
        n_hits = rng.integers(0, k_in + 1, n_q).astype(np.int32)
        n_hits[:2] = [0, k_in]
        ref_s = as_bytes(fm.sort_page(hits, n_hits, values, n_docs, 0, True, first, k, *sort_outputs(n_q, k)))
        ref_g = fm.gather(hits, n_hits, values, n_docs, filled((n_q, k_in, 3), np.int64)).tobytes()
        assert sc.hit_fields(hits, n_hits, out=filled((n_q, k_in, 3), np.int64)).tobytes() == ref_g

        def dev(a):
            return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()

        ptr = lambda a: None if a is None else a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data       # noqa: E731
        back = lambda o: [None if a is None else (a.cpu().numpy() if hasattr(a, "cpu") else a).tobytes() for a in o]   # noqa: E731

        def run_sort(h, n, o, code=0):
            torch.cuda.synchronize()
            assert lib.ss_sort_hits_by_field(sc.h, n_q, k_in, ptr(h), ptr(n), 0, 1, first, k, ptr(o[0]), ptr(o[1]), ptr(o[2])) == code
            ss_ctx.synchronize()
            return back(o)

        def run_gather(h, n, o, code=0):
            torch.cuda.synchronize()
            assert lib.ss_hit_fields(sc.h, n_q, k_in, ptr(h), ptr(n), ptr(o)) == code
            ss_ctx.synchronize()
            return back([o])[0]

        d_hits, d_n = dev(hits), dev(n_hits)
        host_out = lambda: list(sort_outputs(n_q, k))                            # noqa: E731
        dev_out = lambda: [dev(a) for a in sort_outputs(n_q, k)]                # noqa: E731
        g_host = lambda: filled((n_q, k_in, 3), np.int64)                        # noqa: E731
        assert run_sort(d_hits, d_n, dev_out()) == ref_s                         # all device
        assert run_sort(hits, n_hits, host_out()) == ref_s                       # all host
        assert run_sort(d_hits, n_hits, dev_out()) == ref_s                      # mixed
        assert run_sort(hits, d_n, host_out()) == ref_s
        mixed = host_out()
        mixed[0] = dev(mixed[0])
        assert run_sort(d_hits, d_n, mixed) == ref_s
        mixed = dev_out()
        mixed[2] = sort_outputs(n_q, k)[2]
        assert run_sort(hits, d_n, mixed) == ref_s
        for make in (host_out, dev_out):                                         # values_out NULL
            o = make()
            o[2] = None
            assert run_sort(d_hits, d_n, o) == ref_s[:2] + [None]
        assert run_gather(d_hits, d_n, dev(g_host())) == ref_g
        assert run_gather(hits, d_n, g_host()) == ref_g
        assert run_gather(d_hits, n_hits, dev(g_host())) == ref_g
        # a device n_hits outside [0, k_in] is clamped by the kernel; the same array in host memory is refused
        bad = n_hits.copy()
        bad[0], bad[1], bad[5] = -1, k_in + 5, -2 ** 31
        clamped = as_bytes(fm.sort_page(hits, bad, values, n_docs, 0, True, first, k, *sort_outputs(n_q, k), clamp=True))
        assert run_sort(d_hits, dev(bad), dev_out()) == clamped
        assert run_sort(hits, dev(bad), host_out()) == clamped
        assert run_sort(hits, bad, host_out(), code=ERR_INVALID) == as_bytes(sort_outputs(n_q, k))
        g_clamped = fm.gather(hits, bad, values, n_docs, g_host(), clamp=True).tobytes()
        assert run_gather(d_hits, dev(bad), dev(g_host())) == g_clamped
        assert run_gather(hits, dev(bad), g_host()) == g_clamped
        assert run_gather(hits, bad, g_host(), code=ERR_INVALID) == g_host().tobytes()
        # the engine wrapper with device arrays returns them as they are
        o = dev_out()
        got = sc.sort_hits_by_field(d_hits, d_n.view(torch.int32), 0, k, descending=True, first=first, k_in=k_in,
                                    out=(o[0], o[1].view(torch.int32), o[2].view(torch.int64)))
        assert [a.cpu().numpy().tobytes() for a in got] == ref_s
    finally:
        close_all(sc, ti, bi)


def test_refusals_leave_the_outputs_untouched(ss_ctx, world):
    sc, ti, bi = make_scorer(ss_ctx, world["n_docs"], world["title"], world["body"], world["mt"], world["mb"])
    try:
        lib = ss_ctx.lib
        n_docs = world["n_docs"]
        n_words = (n_docs + 31) // 32
        rng = np.random.default_rng(8)
        ptr = lambda a: None if a is None else a.ctypes.data       # noqa: E731
        hits = random_rows(rng, 2, 4, n_docs)
        n_hits = np.array([4, 2], np.int32)
        out = sort_outputs(2, 3)
        g_out = filled((2, 4, 4), np.int64)
        words = filled((2, n_words), np.uint32)
        s_hits, s_n = filled((2, 5), engine.HIT_DTYPE), filled(2, np.int32)
        untouched = as_bytes(list(out) + [g_out, words, s_hits, s_n])
        q_ptr, q_terms = np.array([0, 1, 3], np.uint32), np.array([0, 1, 2], np.uint32)
        one = engine.pack_doc_ranges([[(0, 0, 5)], [(1, 0, 5)]])

        def same():
            assert as_bytes(list(out) + [g_out, words, s_hits, s_n]) == untouched

        def sort(code, handle="sc", n_q=2, k_in=4, h=hits, n=n_hits, field=0, first=0, k=3, o0=out[0], o1=out[1]):
            rc = lib.ss_sort_hits_by_field(sc.h if handle == "sc" else handle, n_q, k_in, ptr(h), ptr(n), field, 0, first, k, ptr(o0), ptr(o1),
                                           ptr(out[2]))
            assert rc == code, (rc, code)
            same()

        def gather(code, handle="sc", n_q=2, k_in=4, h=hits, n=n_hits, o=g_out):
            rc = lib.ss_hit_fields(sc.h if handle == "sc" else handle, n_q, k_in, ptr(h), ptr(n), ptr(o))
            assert rc == code, (rc, code)
            same()

        def masks(code, handle="sc", n_sets=2, rp=one[0], rg=one[1], mid=None, o=words):
            rc = lib.ss_doc_field_masks(sc.h if handle == "sc" else handle, n_sets, ptr(rp), ptr(rg), ptr(mid), ptr(o))
            assert rc == code, (rc, code)
            same()

        def scored(code, handle="sc", n_q=2, rp=one[0], rg=one[1], mid=None, k=5, o0=s_hits, o1=s_n):
            rc = lib.ss_score_topk_filtered(sc.h if handle == "sc" else handle, n_q, ptr(q_ptr), ptr(q_terms), None, None, None, None, ptr(mid),
                                            None, None, None, None, ptr(rp), ptr(rg), k, ptr(o0), ptr(o1))
            assert rc == code, (rc, code)
            same()
        # no table yet: the calls that need one are refused; sets without a clause need none
        for fn in (sort, gather, masks, scored):
            fn(ERR_STATE)
        with pytest.raises(SpaghettiError) as ei:
            sc.sort_hits_by_field(hits, n_hits, 0, 3, out=out)
        assert ei.value.code == ERR_STATE
        same()
        assert lib.ss_scorer_set_doc_fields(sc.h, -1, ptr(world["values"])) == ERR_INVALID
        assert lib.ss_scorer_set_doc_fields(sc.h, 5, ptr(world["values"])) == ERR_UNSUPPORTED
        assert lib.ss_scorer_set_doc_fields(None, 1, ptr(world["values"])) == ERR_INVALID
        sort(ERR_STATE)                                                       # (the refused registrations left no table)
        sc.set_doc_fields(world["values"][:2])
        assert lib.ss_scorer_set_doc_fields(sc.h, 5, ptr(world["values"])) == ERR_UNSUPPORTED      # ... and leave the old one in place
        for fn in (sort, gather, masks, scored):
            fn(ERR_INVALID, handle=None)
        for fn in (sort, gather, scored):
            fn(ERR_INVALID, n_q=-1)
        masks(ERR_INVALID, n_sets=-1)
        for fn in (sort, gather):
            fn(ERR_INVALID, k_in=0)
            fn(ERR_UNSUPPORTED, k_in=1025)
            fn(ERR_INVALID, h=None)
            fn(ERR_INVALID, n=None)
            fn(ERR_INVALID, n=np.array([5, 1], np.int32))
            fn(ERR_INVALID, n=np.array([1, -1], np.int32))
        gather(ERR_INVALID, o=None)
        sort(ERR_INVALID, k=0)
        sort(ERR_UNSUPPORTED, k=1025)
        sort(ERR_INVALID, first=-1)
        sort(ERR_INVALID, field=-1)
        sort(ERR_INVALID, field=2)                                            # two fields registered
        sort(ERR_INVALID, o0=None)
        sort(ERR_INVALID, o1=None)
        scored(ERR_INVALID, k=0)
        scored(ERR_UNSUPPORTED, k=1025)
        scored(ERR_INVALID, o0=None)
        masks(ERR_INVALID, o=None)
        masks(ERR_INVALID, rp=None)
        for fn in (masks, scored):
            fn(ERR_INVALID, rp=np.array([1, 1, 2], np.uint32))               # does not start at 0
            fn(ERR_INVALID, rp=np.array([0, 2, 1], np.uint32))               # decreases
            fn(ERR_INVALID, rg=None)
            fn(ERR_INVALID, rg=engine.pack_doc_ranges([[(0, 0, 5)], [(2, 0, 5)]])[1])       # field 2 of two
            fn(ERR_INVALID, rg=engine.pack_doc_ranges([[(-1, 0, 5)], [(1, 0, 5)]])[1])
            five = engine.pack_doc_ranges([[(0, 0, 5)] * 5, []])
            fn(ERR_UNSUPPORTED, rp=five[0], rg=five[1])
            fn(ERR_INVALID, mid=np.array([0, -1], np.int32))                  # no masks registered
            fn(ERR_INVALID, mid=np.array([-2, -1], np.int32))
        # hits_out overlapping hits
        both = np.concatenate([hits.reshape(-1), hits.reshape(-1)])
        before = both.tobytes()
        for off in (0, 1, 7):
            rc = lib.ss_sort_hits_by_field(sc.h, 2, 4, both.ctypes.data, n_hits.ctypes.data, 0, 0, 0, 3, both[off:].ctypes.data, ptr(out[1]), None)
            assert rc == ERR_INVALID and both.tobytes() == before
            same()
        # nothing to do: SS_OK, nothing written
        sort(0, n_q=0)
        sort(0, n_q=0, h=None, n=None, o0=None, o1=None)
        gather(0, n_q=0)
        masks(0, n_sets=0)
        masks(0, n_sets=0, rp=None, rg=None, o=None)
        scored(0, n_q=0)
        # the same arguments untouched are accepted, and after clearing the table refused again
        check_sort(sc, hits, n_hits, world["values"], n_docs, 1, False, 0, 3)
        assert lib.ss_doc_field_masks(sc.h, 2, ptr(one[0]), ptr(one[1]), None, ptr(words)) == 0
        assert words.tobytes() == fm.set_words(world["values"], n_docs, [[(0, 0, 5)], [(1, 0, 5)]]).tobytes()
        sc.set_doc_fields(None)
        words[:] = filled(words.shape, np.uint32)
        for fn in (sort, gather, masks, scored):
            fn(ERR_STATE)
    finally:
        close_all(sc, ti, bi)


def test_chain_score_filtered_sort_explain_on_one_stream(ss_ctx, world, scorer):
    """score (filtered) -> sort newest first -> read the fields -> explain, device buffers throughout, one synchronise at the end"""
    import torch
    sc = scorer[0]
    lib = ss_ctx.lib
    n_docs = world["n_docs"]
    rng = np.random.default_rng(14)
    n_q, k_window, k, t_stride = 12, 200, 10, 4
    q_ptr, q_terms = queries(rng, n_q, world["n_terms"])
    clauses = [[(0, 0, 499)] if q % 2 else [(0, 0, 499), (1, I64_MIN, 3000)] for q in range(n_q)]
    rp, rg = engine.pack_doc_ranges(clauses)
    buf = lambda n: torch.full((n,), FILL, dtype=torch.uint8, device="cuda")           # noqa: E731
    d_rows, d_n, d_page, d_pn, d_vals = buf(n_q * k_window * 40), buf(n_q * 4), buf(n_q * k * 40), buf(n_q * 4), buf(n_q * k * 8)
    d_fields, d_exp = buf(n_q * k * 4 * 8), buf(n_q * k * t_stride * 16)
    torch.cuda.synchronize()
    assert lib.ss_score_topk_filtered(sc.h, n_q, q_ptr.ctypes.data, q_terms.ctypes.data, None, None, None, None, None, None, None, None,
                                      None, rp.ctypes.data, rg.ctypes.data, k_window, d_rows.data_ptr(), d_n.data_ptr()) == 0
    assert lib.ss_sort_hits_by_field(sc.h, n_q, k_window, d_rows.data_ptr(), d_n.data_ptr(), 0, 1, 0, k, d_page.data_ptr(), d_pn.data_ptr(),
                                     d_vals.data_ptr()) == 0
    assert lib.ss_hit_fields(sc.h, n_q, k, d_page.data_ptr(), d_pn.data_ptr(), d_fields.data_ptr()) == 0
    assert lib.ss_explain_hits(sc.h, n_q, q_ptr.ctypes.data, q_terms.ctypes.data, k, d_page.data_ptr(), d_pn.data_ptr(), t_stride,
                               d_exp.data_ptr()) == 0
    ss_ctx.synchronize()
    rows, n_rows = check_filtered(sc, world, q_ptr, q_terms, clauses, k_window)
    got_rows = d_rows.cpu().numpy().view(engine.HIT_DTYPE).reshape(n_q, k_window)
    assert d_n.cpu().numpy().view(np.int32).tolist() == n_rows.tolist() and n_rows.max() > k
    assert all(got_rows[q, :n_rows[q]].tobytes() == rows[q, :n_rows[q]].tobytes() for q in range(n_q))
    page = fm.sort_page(rows, n_rows, world["values"], n_docs, 0, True, 0, k, *sort_outputs(n_q, k))
    assert [d_page.cpu().numpy().tobytes(), d_pn.cpu().numpy().tobytes(), d_vals.cpu().numpy().tobytes()] == as_bytes(page)
    assert d_fields.cpu().numpy().tobytes() == fm.gather(page[0], page[1], world["values"], n_docs, filled((n_q, k, 4), np.int64)).tobytes()
    exp = sc.explain_hits(q_ptr, q_terms, page[0], page[1], t_stride=t_stride, out=filled((n_q, k, t_stride), engine.TERM_MATCH_DTYPE))
    assert d_exp.cpu().numpy().tobytes() == exp.tobytes()
    vals = page[2]
    assert all((np.diff(vals[q, :page[1][q]]) <= 0).all() for q in range(n_q))            # newest first

