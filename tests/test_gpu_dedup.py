"""GPU parity: MinHash signatures (ss_index_build_signatures / _drop_signatures / _read_signatures) and the near-duplicate walk
(ss_dedup_hits) vs the numpy model of tests/dedup_model.py.  Integer results only: every comparison is bit-exact, and the dedup
outputs start from 0xA5 bytes so that an entry the call must not write is checked with the ones it must."""
import ctypes
import os
import re

import numpy as np
import pytest

from spaghettisearch_amd import SpaghettiError, engine, synth
from tests import collapse_model as cm
from tests import dedup_model as dm
from tests import doc_view_model as dvm
from tests.test_gpu_score import close_all, make_scorer

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE, ERR_UNSUPPORTED = 1, 6, 7
FILL = 0xA5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "index_300x80.npz")
SRC = os.path.join(ROOT, "spaghettisearch_amd", "csrc", "dedup.hip")
N_SLOTS = 16


def kernel_constants():
    """the row-class cut-overs of k_doc_signatures and the tile of k_dedup_hits, read from the source"""
    text = open(SRC).read()
    c = {m.group(1): int(m.group(2)) for m in re.finditer(r"^constexpr uint32_t (\w+) = (\d+);", text, re.M)}
    assert {"SG_GROUP_MAX", "SG_WAVE_MAX", "SG_CHUNK", "DD_TILE"} <= set(c)
    return c


def table_from_rows(rows, n_terms):
    """term-major CSR (term_ptr, post_doc, post_w) of docs given as term arrays"""
    doc = np.concatenate([np.full(len(r), d, np.uint32) for d, r in enumerate(rows)] + [np.zeros(0, np.uint32)])
    term = np.concatenate([np.asarray(r, np.uint32) for r in rows] + [np.zeros(0, np.uint32)])
    order = np.lexsort((doc, term))
    term_ptr = np.concatenate([[0], np.cumsum(np.bincount(term, minlength=n_terms))]).astype(np.uint64)
    return term_ptr, doc[order].astype(np.uint32), np.ones(len(order), np.float32)


def filled(shape, dtype):
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return np.frombuffer(bytes([FILL]) * n, dtype=dtype).reshape(shape).copy()


def outputs(n_q, k, similar=True, kept=True):
    return (filled((n_q, k), engine.HIT_DTYPE), filled(n_q, np.int32), filled((n_q, k), np.uint32) if similar else None,
            filled(n_q, np.int32) if kept else None)


def as_bytes(out):
    return [None if a is None else np.ascontiguousarray(a).tobytes() for a in out]


def random_rows(rng, n_q, k_in):
    """rows of random BYTES (NaN, -0.0, anything in _pad and the scores; not sorted by anything)"""
    return np.frombuffer(rng.bytes(n_q * k_in * 40), dtype=engine.HIT_DTYPE).reshape(n_q, k_in).copy()


# ---------------------------------------------------------------- signatures

@pytest.fixture(scope="module")
def sig_world():
    """A view with rows of every class of k_doc_signatures, both sides of every cut-over, 0 and n_terms - 1 among the term ids."""
    c = kernel_constants()
    gm, wm, ch = c["SG_GROUP_MAX"], c["SG_WAVE_MAX"], c["SG_CHUNK"]
    n_terms = 70000
    rng = np.random.default_rng(41)
    lens = [0, 1, 2, 63, 64, 65, 255, 256, 257, gm - 1, gm, gm + 1, wm - 1, wm, wm + 1, ch - 1, ch, ch + 1, 5000, 2 * ch, 2 * ch + 1]
    lens += rng.integers(0, gm + 9, 2990).tolist()                              # the bulk: short rows, many blocks, n_docs no multiple of 8
    lens = np.array(lens)[rng.permutation(len(lens))].tolist() + [wm - 3]       # (the last doc: a wave row at the end of the table)
    rows = []
    for d, n in enumerate(lens):
        r = rng.choice(n_terms, n, replace=False)
        if n >= 2 and d % 3 == 0:
            r[:2] = [0, n_terms - 1]
            r = np.unique(r)                                                    # (may be one short of n: the classes are asserted below)
        rows.append(np.sort(r).astype(np.uint32))
    n_docs = len(rows)
    tab = table_from_rows(rows, n_terms)
    view = dvm.doc_view(*tab, n_docs)
    got_lens = np.diff(view[0].astype(np.int64))
    assert n_docs % 8 and view[1].min() == 0 and view[1].max() == n_terms - 1
    for want in (0, 1, 2, 63, 64, 65, 255, 256, 257, gm, gm + 1, wm, wm + 1, ch, ch + 1, 5000, 2 * ch, 2 * ch + 1):
        assert (got_lens == want).any(), want
    # every class: a group's row, a wave's row, one chunk, two chunks, three chunks
    assert (got_lens <= gm).any() and ((got_lens > gm) & (got_lens <= wm)).any() and ((got_lens > wm) & (got_lens <= ch)).any()
    assert ((got_lens > ch) & (got_lens <= 2 * ch)).any() and (got_lens > 2 * ch).any()
    return {"n_docs": n_docs, "n_terms": n_terms, "tab": tab, "view": view, "refs": {}}


def sig_ref(w, n_slots):
    if n_slots not in w["refs"]:
        w["refs"][n_slots] = dm.signatures(w["view"][0], w["view"][1], n_slots)
    return w["refs"][n_slots]


@pytest.mark.parametrize("n_slots", [4, 16, 32])
def test_signatures_equal_the_model(ss_ctx, sig_world, n_slots):
    w = sig_world
    idx = engine.InvertedIndex(ss_ctx, w["n_docs"], *w["tab"])
    try:
        idx.build_doc_view()
        idx.build_signatures(n_slots)
        all_docs = np.arange(w["n_docs"], dtype=np.uint32)
        got = idx.read_signatures(all_docs)
        ref = sig_ref(w, n_slots)
        assert got.shape == ref.shape and got.dtype == np.uint32
        bad = np.nonzero((got != ref).any(axis=1))[0]
        assert got.tobytes() == ref.tobytes(), (bad[:10], np.diff(w["view"][0].astype(np.int64))[bad[:10]])
        empty = np.diff(w["view"][0].astype(np.int64)) == 0
        assert empty.any() and ((got == dm.SIG_EMPTY).all(axis=1) == empty).all()
        idx.build_signatures(n_slots)                                           # two builds: identical bytes
        assert idx.read_signatures(all_docs).tobytes() == ref.tobytes()
    finally:
        idx.close()


def test_signature_lifetime_and_errors(ss_ctx, sig_world):
    import torch
    w = sig_world
    n_docs = w["n_docs"]
    idx = engine.InvertedIndex(ss_ctx, n_docs, *w["tab"])
    lib = ss_ctx.lib
    some = np.array([0, n_docs - 1, 5, 5, 17], np.uint32)

    def none():
        for call in (lambda: idx.read_signatures(some), idx.drop_signatures):
            with pytest.raises(SpaghettiError) as ei:
                call()
            assert ei.value.code == ERR_STATE

    def build(n_slots=N_SLOTS):
        idx.build_doc_view()
        idx.build_signatures(n_slots)
    try:
        none()
        assert lib.ss_index_build_signatures(idx.h, 8) == ERR_STATE             # no doc view
        idx.build_doc_view()
        for n_slots, code in ((0, ERR_INVALID), (-4, ERR_INVALID), (1, ERR_INVALID), (3, ERR_INVALID), (5, ERR_INVALID), (30, ERR_INVALID),
                              (33, ERR_UNSUPPORTED), (36, ERR_UNSUPPORTED), (2 ** 31 - 1, ERR_UNSUPPORTED)):
            assert lib.ss_index_build_signatures(idx.h, n_slots) == code, n_slots
        assert lib.ss_index_build_signatures(None, 8) == ERR_INVALID
        none()
        idx.build_signatures(N_SLOTS)
        ref = sig_ref(w, N_SLOTS)
        assert idx.read_signatures(some).tobytes() == ref[some].tobytes()
        assert lib.ss_index_build_signatures(idx.h, 5) == ERR_INVALID           # a refused build leaves the signatures that exist
        assert idx.read_signatures(some).tobytes() == ref[some].tobytes()
        idx.build_signatures(4)                                                 # another n_slots replaces them
        assert idx.read_signatures(some).tobytes() == sig_ref(w, 4)[some].tobytes()
        idx.build_signatures(N_SLOTS)
        # host and device pointers
        d_docs = torch.from_numpy(some.view(np.int32).copy()).cuda()
        d_out = torch.full((len(some) * N_SLOTS,), -1515870811, dtype=torch.int32, device="cuda")
        assert idx.read_signatures(d_docs, out=d_out) is d_out
        assert d_out.cpu().numpy().tobytes() == ref[some].tobytes()
        assert idx.read_signatures(d_docs).tobytes() == ref[some].tobytes()
        d_out.fill_(-1515870811)
        assert idx.read_signatures(some, out=d_out).cpu().numpy().tobytes() == ref[some].tobytes()
        n_slots_out = ctypes.c_int32(0)
        assert lib.ss_index_read_signatures(idx.h, 0, None, None, ctypes.byref(n_slots_out)) == 0 and n_slots_out.value == N_SLOTS
        assert lib.ss_index_read_signatures(idx.h, 0, None, None, None) == 0
        # a doc outside the table: refused, sig_out untouched, in host and in device memory
        bad = np.array([1, n_docs, 2], np.uint32)
        out = filled((3, N_SLOTS), np.uint32)
        assert lib.ss_index_read_signatures(idx.h, 3, bad.ctypes.data, out.ctypes.data, None) == ERR_INVALID
        assert out.tobytes() == filled((3, N_SLOTS), np.uint32).tobytes()
        d_out.fill_(7)
        assert lib.ss_index_read_signatures(idx.h, 3, torch.from_numpy(bad.view(np.int32).copy()).cuda().data_ptr(), d_out.data_ptr(), None) == ERR_INVALID
        assert (d_out.cpu().numpy() == 7).all()
        assert lib.ss_index_read_signatures(idx.h, 3, None, out.ctypes.data, None) == ERR_INVALID
        assert lib.ss_index_read_signatures(idx.h, 3, bad.ctypes.data, None, None) == ERR_INVALID
        # dropping or rebuilding the view leaves the signatures
        idx.drop_doc_view()
        assert idx.read_signatures(some).tobytes() == ref[some].tobytes()
        idx.build_doc_view()
        assert idx.read_signatures(some).tobytes() == ref[some].tobytes()
        idx.set_weighted(np.ones(n_docs))
        assert idx.read_signatures(some).tobytes() == ref[some].tobytes()
        # every call that frees them
        idx.tfidf_build(n_docs)
        none()
        build()
        idx.apply_delta(del_docs=np.array([5], np.uint32), add=(np.array([3, 69999], np.uint32), np.array([5, 5], np.uint32), np.array([0.5, 0.5], np.float32)))
        none()
        build()
        got = idx.read_signatures(some)
        assert got[2].tolist() == dm.row_signature([3, 69999], N_SLOTS).tolist() and got[0].tobytes() == ref[0].tobytes()   # of the updated table
        idx.resize(n_docs + 10, w["n_terms"])
        none()
        build()
        assert (idx.read_signatures(np.array([n_docs + 9], np.uint32)) == dm.SIG_EMPTY).all()
        idx.drop_signatures()
        none()
    finally:
        idx.close()


# ---------------------------------------------------------------- the walk

N_FAM, N_VAR, BASE_LEN = 48, 12, 40


@pytest.fixture(scope="module")
def dup_world():
    """Docs made from base term sets plus variants: variant v of family f changes 0, 0, 1, 1, 2, 3, 5, 8, 12, 16, 20 or 28 of the base's
    40 terms, so the pairs inside a family agree in anything from a few slots to all of them.  Behind them docs without body terms."""
    rng = np.random.default_rng(12)
    n_terms = 20000
    changes = [0, 0, 1, 1, 2, 3, 5, 8, 12, 16, 20, 28]
    rows = []
    for f in range(N_FAM):
        base = rng.choice(n_terms, BASE_LEN, replace=False)
        for v in range(N_VAR):
            r = base.copy()
            r[rng.choice(BASE_LEN, changes[v], replace=False)] = rng.choice(n_terms, changes[v], replace=False)
            rows.append(np.unique(r).astype(np.uint32))
    n_fam_docs = len(rows)
    rows += [np.zeros(0, np.uint32)] * 8                                        # docs n_fam_docs .. + 7: no body terms
    rows += [rng.choice(n_terms, 30, replace=False).astype(np.uint32) for _ in range(1500)]   # unrelated pages
    n_docs = len(rows)
    body = table_from_rows(rows, n_terms)
    sig = dm.signatures(*dvm.doc_view(*body, n_docs)[:2], N_SLOTS)
    return {"n_docs": n_docs, "n_terms": n_terms, "body": body, "sig": sig, "n_fam_docs": n_fam_docs, "empty": n_fam_docs + np.arange(8)}


def make_window(w, rng, n):
    """n window docs: mostly family docs (the first 128 rows from six families only, so that a short window holds every case), some
    unrelated, some without a signature (empty body, outside the table), each kind more than once"""
    docs = np.empty(n, np.int64)
    for j in range(n):
        fams = 6 if j < 128 else N_FAM
        u = rng.random()
        if u < 0.80:
            docs[j] = rng.integers(0, fams) * N_VAR + rng.integers(0, N_VAR)
        elif u < 0.88:
            docs[j] = rng.integers(w["n_fam_docs"] + 8, w["n_docs"])
        elif u < 0.94:
            docs[j] = rng.choice(w["empty"][:2])
        else:
            docs[j] = rng.choice([w["n_docs"], w["n_docs"] + 1, 0xFFFFFFFF, 0x80000000])
    return docs.astype(np.uint32)


def assert_cases(w, docs, min_match, tile):
    """the model says the window holds every case the definition distinguishes"""
    m = dm.fast_match(docs, w["sig"])
    kept, leader, similar = dm.walk(m, min_match)
    n = len(docs)
    is_kept = np.zeros(n, bool)
    is_kept[kept] = True
    lead = np.array(leader)
    j_idx = np.arange(n)
    dropped = np.nonzero(~is_kept)[0]
    assert len(dropped) and len(kept) > 1
    # decided at the bound: a duplicate whose best kept match is exactly min_match; a kept row that misses some kept row by one
    upper = np.triu(np.ones((n, n), bool), 1) & is_kept[:, None]                # (i, j): i < j, i kept
    assert any(m[lead[j], j] == min_match and (m[:j, j][is_kept[:j]] <= min_match).all() for j in dropped)
    assert (upper & (m == min_match - 1) & is_kept[None, :]).any()
    if min_match < N_SLOTS:
        # (all slots equal is an equivalence: at min_match = n_slots two kept rows never match the same row and a dropped row's matches
        # are its leader's, so neither a shielded chain nor a second candidate leader can exist there)
        shield = [(b, c) for b in dropped for c in kept if c > b and m[b, c] >= min_match]
        assert shield                                                           # a ~ b, b ~ c, b dropped, c kept all the same
        assert any((upper[:, j] & (m[:, j] >= min_match)).sum() >= 2 for j in dropped)       # two candidate leaders
    assert ((lead // tile < j_idx // tile) & ~is_kept).any() and ((lead // tile == j_idx // tile) & ~is_kept).any()
    own = m.diagonal() < 0
    docs64 = docs.astype(np.int64)
    assert (docs64 >= w["n_docs"]).sum() >= 2 and np.isin(docs64, w["empty"]).sum() >= 2 and is_kept[own].all()
    assert all(similar[j] == 1 for j in np.nonzero(own)[0])
    twice = [d for d in set(docs64.tolist()) if (docs64 == d).sum() >= 2]
    assert any(d < w["n_docs"] and not own[docs64 == d].any() for d in twice)                # the same doc twice with a signature ..
    assert any(own[docs64 == d].all() for d in twice)                                        # .. and twice without one
    for d in twice:
        rows_d = np.nonzero(docs64 == d)[0]
        assert is_kept[rows_d].all() if own[rows_d[0]] else not is_kept[rows_d[1:]].any()
    return len(kept)


@pytest.fixture(scope="module")
def dup_scorer(ss_ctx, dup_world):
    w = dup_world
    one = (np.array([0, 1], np.uint64), np.array([0], np.uint32), np.array([1.0], np.float32))
    title = (np.concatenate([one[0], np.ones(w["n_terms"] - 1, np.uint64)]), one[1], one[2])
    sc, ti, bi = make_scorer(ss_ctx, w["n_docs"], title, w["body"], np.ones(w["n_docs"]), np.ones(w["n_docs"]))
    bi.build_doc_view()
    bi.build_signatures(N_SLOTS)
    yield sc, ti, bi
    close_all(sc, ti, bi)


@pytest.mark.parametrize("min_match", [1, N_SLOTS // 2, N_SLOTS])
@pytest.mark.parametrize("k_in", [128, 1024])
def test_dedup_equals_the_model(dup_world, dup_scorer, k_in, min_match):
    """both instances of k_dedup_hits: windows of 0 .. 128 rows at k_in = 128, of 65 .. 1024 rows at k_in = 1024"""
    w, sc = dup_world, dup_scorer[0]
    tile = kernel_constants()["DD_TILE"]
    assert tile == 64
    rng = np.random.default_rng(1000 + k_in)
    sizes = [0, 1, 2, 63, 64, 65, 128] if k_in == 128 else [65, 129, 1000, 1024]
    hits = random_rows(rng, len(sizes), k_in)
    full = make_window(w, rng, k_in)
    hits["doc"][:] = full                                                       # every window a prefix of the full one
    n_hits = np.array(sizes, np.int32)
    assert bi_signatures_match(dup_scorer[2], w)
    n_kept = assert_cases(w, full, min_match, tile)                             # the full window holds every case
    assert 2 < n_kept < k_in
    for first in (0, n_kept // 2, n_kept, n_kept + 3):
        for k in (k_in, 50):
            for both in (True, False):
                got = sc.dedup_hits(hits, n_hits, min_match, k, first=first, out=outputs(len(sizes), k, both, both))
                ref = dm.dedup(hits, n_hits, w["sig"], min_match, first, k, *outputs(len(sizes), k, both, both))
                assert as_bytes(got) == as_bytes(ref), (first, k, both)
    got = sc.dedup_hits(hits, n_hits, min_match, k_in, out=outputs(len(sizes), k_in))
    assert int(got[3][-1]) == n_kept == int(got[1][-1])
    assert int(got[2][-1, :n_kept].sum()) == k_in                               # every row of the window is led by one kept row
    if k_in == 128:
        assert got[1].tolist()[:2] == [0, 1] == got[3].tolist()[:2]             # the windows of no row and of one


def bi_signatures_match(bi, w):
    docs = np.arange(w["n_docs"], dtype=np.uint32)
    return bi.read_signatures(docs).tobytes() == w["sig"].tobytes()


def test_pointer_placements_and_clamping(ss_ctx, dup_world, dup_scorer):
    import torch
    w, sc = dup_world, dup_scorer[0]
    lib = ss_ctx.lib
    rng = np.random.default_rng(4)
    n_q, k_in, mm, first, k = 9, 130, 6, 3, 40
    hits = random_rows(rng, n_q, k_in)
    for q in range(n_q):
        hits["doc"][q] = make_window(w, rng, k_in)
    n_hits = rng.integers(0, k_in + 1, n_q).astype(np.int32)
    n_hits[:2] = [k_in, 0]
    ref = as_bytes(dm.dedup(hits, n_hits, w["sig"], mm, first, k, *outputs(n_q, k)))

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()

    def run(h, n, o, code=0):
        ptr = lambda a: None if a is None else a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data       # noqa: E731
        torch.cuda.synchronize()
        rc = lib.ss_dedup_hits(sc.h, n_q, k_in, ptr(h), ptr(n), mm, first, k, ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(o[3]))
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
    assert run(d_hits, d_n, mixed) == ref                                    # device rows and n_kept, host counts and similar
    mixed = dev_out()
    mixed[0], mixed[3] = outputs(n_q, k)[0], outputs(n_q, k)[3]
    assert run(hits, d_n, mixed) == ref
    for drop in ((2,), (3,), (2, 3)):                                        # similar_out / n_kept_out NULL
        for make in (host_out, dev_out):
            o = make()
            for i in drop:
                o[i] = None
            assert run(d_hits if make is dev_out else hits, d_n, o) == [None if i in drop else ref[i] for i in range(4)]
    # a device n_hits outside [0, k_in] is clamped by the kernel; the same array in host memory is refused
    bad = n_hits.copy()
    bad[0], bad[1], bad[5] = -1, k_in + 5, -2 ** 31
    clamped = as_bytes(dm.dedup(hits, bad, w["sig"], mm, first, k, *outputs(n_q, k), clamp=True))
    assert run(d_hits, dev(bad), dev_out()) == clamped
    assert run(hits, dev(bad), host_out()) == clamped
    assert run(hits, bad, host_out(), code=ERR_INVALID) == as_bytes(outputs(n_q, k))
    # the engine wrapper with device arrays returns them as they are
    o = dev_out()
    got = sc.dedup_hits(d_hits, d_n.view(torch.int32), mm, k, first=first, k_in=k_in,
                        out=(o[0], o[1].view(torch.int32), o[2].view(torch.int32), o[3].view(torch.int32)))
    assert [a.cpu().numpy().tobytes() for a in got] == ref


def test_refusals_leave_the_outputs_untouched(ss_ctx, dup_world):
    w = dup_world
    one = (np.array([0, 1], np.uint64), np.array([0], np.uint32), np.array([1.0], np.float32))
    title = (np.concatenate([one[0], np.ones(w["n_terms"] - 1, np.uint64)]), one[1], one[2])
    sc, ti, bi = make_scorer(ss_ctx, w["n_docs"], title, w["body"], np.ones(w["n_docs"]), np.ones(w["n_docs"]))
    try:
        lib = ss_ctx.lib
        rng = np.random.default_rng(8)
        hits = random_rows(rng, 2, 4)
        hits["doc"] = [[0, 1, 2, 3], [12, 13, 0, 600]]
        n_hits = np.array([4, 2], np.int32)
        out = outputs(2, 3)
        untouched = as_bytes(outputs(2, 3))
        ptr = lambda a: None if a is None else a.ctypes.data       # noqa: E731

        def call(code, handle="sc", n_q=2, k_in=4, h=hits, n=n_hits, mm=1, first=0, k=3, o0=out[0], o1=out[1]):
            rc = lib.ss_dedup_hits(sc.h if handle == "sc" else handle, n_q, k_in, ptr(h), ptr(n), mm, first, k, ptr(o0), ptr(o1),
                                   ptr(out[2]), ptr(out[3]))
            assert rc == code, (rc, code)
            assert as_bytes(out) == untouched
        call(ERR_STATE)                                                       # no signatures yet
        ti.build_doc_view()
        ti.build_signatures(8)                                                # the TITLE table's signatures do not count
        call(ERR_STATE)
        with pytest.raises(SpaghettiError) as ei:
            sc.dedup_hits(hits, n_hits, 1, 3, out=out)
        assert ei.value.code == ERR_STATE and as_bytes(out) == untouched
        bi.build_doc_view()
        bi.build_signatures(8)
        call(ERR_INVALID, handle=None)
        call(ERR_INVALID, n_q=-1)
        call(ERR_INVALID, mm=0)
        call(ERR_INVALID, mm=-3)
        call(ERR_INVALID, mm=9)                                               # more than the signatures' slots
        call(ERR_INVALID, first=-1)
        call(ERR_INVALID, k=0)
        call(ERR_INVALID, k_in=0)
        call(ERR_INVALID, o0=None)
        call(ERR_INVALID, o1=None)
        call(ERR_INVALID, h=None)
        call(ERR_INVALID, n=None)
        call(ERR_UNSUPPORTED, k=1025)
        call(ERR_UNSUPPORTED, k_in=1025)
        call(ERR_INVALID, n=np.array([5, 1], np.int32))
        call(ERR_INVALID, n=np.array([1, -1], np.int32))
        both = np.concatenate([hits.reshape(-1), hits.reshape(-1)])           # hits_out overlapping hits
        before = both.tobytes()
        for off in (0, 1, 7):
            rc = lib.ss_dedup_hits(sc.h, 2, 4, both.ctypes.data, n_hits.ctypes.data, 1, 0, 3, both[off:].ctypes.data, ptr(out[1]), None, None)
            assert rc == ERR_INVALID and both.tobytes() == before and as_bytes(out) == untouched
        call(0, n_q=0)                                                        # nothing to do: SS_OK, nothing written
        call(0, n_q=0, h=None, n=None, o0=None, o1=None)
        got = sc.dedup_hits(hits, n_hits, 8, 3, out=outputs(2, 3))            # the same arguments untouched are accepted
        assert as_bytes(got) == as_bytes(dm.dedup(hits, n_hits, w["sig"][:, :8], 8, 0, 3, *outputs(2, 3)))
        bi.drop_signatures()
        call(ERR_STATE)
    finally:
        close_all(sc, ti, bi)


def test_chain_score_dedup_collapse_explain_on_one_stream(ss_ctx):
    """score -> dedup -> collapse -> explain with device buffers, nothing waits in between; against the same four calls one by one
    through host memory, and the dedup step against the model"""
    import torch
    z = np.load(GOLDEN)
    n_docs = int(z["n_docs"])
    title, body = (z["t_ptr"], z["t_doc"], z["t_w"]), (z["b_ptr"], z["b_doc"], z["b_w"])
    sc, ti, bi = make_scorer(ss_ctx, n_docs, title, body, z["t_mag"], z["b_mag"])
    try:
        lib = ss_ctx.lib
        bi.build_doc_view()
        bi.build_signatures(N_SLOTS)
        sig = dm.signatures(*dvm.doc_view(*body, n_docs)[:2], N_SLOTS)
        rng = np.random.default_rng(6)
        group = rng.integers(0, 40, n_docs).astype(np.uint32)
        sc.set_doc_groups(group)
        rows_q = [[0, 1, 2], [3], [5, 9, 20, 3], [0xFFFFFFFF], [40, 41, 42, 43, 44, 45], [0]]
        q_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows_q])]).astype(np.uint32)
        q_terms = np.array([t for r in rows_q for t in r], np.uint32)
        n_q, k_w, mm, k_d, g, k, t_stride = len(rows_q), 200, 2, 150, 2, 20, 6
        buf = lambda n: torch.full((n,), FILL, dtype=torch.uint8, device="cuda")     # noqa: E731
        d = {"rows": buf(n_q * k_w * 40), "n_rows": buf(n_q * 4), "dd": buf(n_q * k_d * 40), "n_dd": buf(n_q * 4), "sim": buf(n_q * k_d * 4),
             "dkept": buf(n_q * 4), "page": buf(n_q * k * 40), "n_page": buf(n_q * 4), "same": buf(n_q * k * 4), "ckept": buf(n_q * 4),
             "exp": buf(n_q * k * t_stride * 16)}
        torch.cuda.synchronize()
        p = {name: t.data_ptr() for name, t in d.items()}
        assert lib.ss_score_topk(sc.h, n_q, q_ptr.ctypes.data, q_terms.ctypes.data, None, None, k_w, p["rows"], p["n_rows"]) == 0
        assert lib.ss_dedup_hits(sc.h, n_q, k_w, p["rows"], p["n_rows"], mm, 0, k_d, p["dd"], p["n_dd"], p["sim"], p["dkept"]) == 0
        assert lib.ss_collapse_hits(sc.h, n_q, k_d, p["dd"], p["n_dd"], g, 1, k, p["page"], p["n_page"], p["same"], p["ckept"]) == 0
        assert lib.ss_explain_hits(sc.h, n_q, q_ptr.ctypes.data, q_terms.ctypes.data, k, p["page"], p["n_page"], t_stride, p["exp"]) == 0
        ss_ctx.synchronize()
        rows, n_rows = sc.score_topk(q_ptr, q_terms, k_w)
        dd = sc.dedup_hits(rows, n_rows, mm, k_d, out=outputs(n_q, k_d))
        assert as_bytes(dd) == as_bytes(dm.dedup(rows, n_rows, sig, mm, 0, k_d, *outputs(n_q, k_d)))
        assert (dd[3] < n_rows).any() and n_rows[3] == 0                       # something was dropped at all
        o = outputs(n_q, k)
        page = sc.collapse_hits(dd[0], dd[1], g, k, first=1, out=o)
        assert as_bytes(page) == as_bytes(cm.collapse(dd[0], dd[1], group, g, 1, k, *outputs(n_q, k)))
        exp = np.frombuffer(bytes([FILL]) * (n_q * k * t_stride * 16), dtype=engine.TERM_MATCH_DTYPE).reshape(n_q, k, t_stride).copy()
        exp = sc.explain_hits(q_ptr, q_terms, page[0], page[1], t_stride=t_stride, out=exp)
        got = {name: t.cpu().numpy().tobytes() for name, t in d.items()}
        assert [got["dd"], got["n_dd"], got["sim"], got["dkept"]] == as_bytes(dd)
        assert [got["page"], got["n_page"], got["same"], got["ckept"]] == as_bytes(page)
        assert got["exp"] == exp.tobytes() and got["n_rows"] == n_rows.tobytes()
    finally:
        close_all(sc, ti, bi)
