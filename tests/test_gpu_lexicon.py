"""GPU parity: the term lexicon (ss_lexicon_*) vs the Python model (tests/lexicon_model.py).  Every comparison is tobytes() on whole
output arrays that start from 0xA5 bytes, so an entry the call must not write is checked with the ones it must.  The vocabularies are
at most 4096 random words of length 0 .. 12 over the alphabet a b c 0xC3 0xA9 (near neighbours, duplicates and high bytes are dense)
plus hand-placed words.
"""
import ctypes as C

import numpy as np
import pytest

from spaghettisearch_amd import SpaghettiError, engine
from tests import lexicon_model as lm
from tests.test_lexicon_cpu import random_words

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = 1, 7
FILL = 0xA5
W64 = b"abcab" * 12 + b"abca"                             # 64 bytes: the longest word that can be a candidate
HAND = [W64, W64 + b"b", b"abc", b"abc", b"ab\xff", b"ab\x00", b"ab", b"pagerank", b"apgerank", b"pageranK", b"pagerakn",
        b"", b"a", b"\xc3\xa9", W64[:63], W64[:62] + b"ba"]


def filled(shape, dtype):
    return np.frombuffer(bytes([FILL]) * (int(np.prod(shape)) * np.dtype(dtype).itemsize), dtype=dtype).reshape(shape).copy()


def gpu_prefix(lx, prefixes, k, first=0, with_match=True):
    n_q = len(prefixes)
    out = (filled((n_q, k), np.uint32), filled((n_q,), np.int32), filled((n_q,), np.uint64) if with_match else None)
    return lx.prefix(prefixes, k, first, out=out)


ORDERS = {}                                               # the model's order of a vocabulary, computed once


def model_prefix(words, prefixes, k, first=0):
    n_q = len(prefixes)
    if id(words) not in ORDERS:
        ORDERS[id(words)] = (words, lm.order(words))
    return lm.prefix(words, prefixes, first, k, filled((n_q, k), np.uint32), filled((n_q,), np.int32), filled((n_q,), np.uint64),
                     od=ORDERS[id(words)][1])


def gpu_suggest(lx, queries, max_dist, m, min_freq, with_dist=True):
    n_q = len(queries)
    out = (filled((n_q, m), np.uint32), filled((n_q, m), np.int32) if with_dist else None, filled((n_q,), np.int32))
    return lx.suggest(queries, max_dist, m, min_freq, out=out)


def model_suggest(words, freq, queries, max_dist, m, min_freq):
    n_q = len(queries)
    return lm.suggest(words, freq, queries, max_dist, min_freq, m, filled((n_q, m), np.uint32), filled((n_q, m), np.int32),
                      filled((n_q,), np.int32))


def same(got, want):
    for g, w in zip(got, want):
        if g is not None:
            assert g.tobytes() == w.tobytes()


@pytest.fixture(scope="module")
def world():
    """4000 random words + the hand-placed ones, a Zipf-like freq with many ties and zeros; model rows are computed once per key"""
    words = random_words(4000, seed=11) + HAND
    rng = np.random.default_rng(12)
    freq = (rng.zipf(1.5, len(words)) % 50).astype(np.uint32)
    return {"words": words, "freq": freq, "ref": {}}


@pytest.fixture()
def lex(ss_ctx, world):
    lx = engine.Lexicon(ss_ctx, world["words"], world["freq"])
    yield lx
    lx.close()
    ss_ctx.set_option("lexicon.chunk_terms", None)


def ref_suggest(world, queries, max_dist, m, min_freq, freq=None):
    key = (tuple(queries), max_dist, m, min_freq, None if freq is None else freq.tobytes())
    if key not in world["ref"]:
        world["ref"][key] = model_suggest(world["words"], world["freq"] if freq is None else freq, queries, max_dist, m, min_freq)
    return world["ref"][key]


# ---- 1. order
def test_order_equals_the_model(lex, world):
    assert lex.info() == (len(world["words"]), sum(len(w) for w in world["words"]))
    assert lex.order().tobytes() == lm.order(world["words"]).tobytes()


@pytest.mark.parametrize("words", [[], [b"solo"], [b""], [b"same"] * 70], ids=["none", "one", "one-empty", "all-equal"])
def test_order_of_tiny_vocabularies(ss_ctx, words):
    lx = engine.Lexicon(ss_ctx, words)
    try:
        assert lx.order(filled((len(words),), np.uint32)).tobytes() == lm.order(words).tobytes()
        same(gpu_prefix(lx, [b"", b"s", b"same", b"t"], 7), model_prefix(words, [b"", b"s", b"same", b"t"], 7))
        same(gpu_suggest(lx, [b"", b"solo", b"sam"], 1, 5, 0), model_suggest(words, None, [b"", b"solo", b"sam"], 1, 5, 0))
    finally:
        lx.close()


# ---- 2. prefix
def test_empty_prefix_paged_until_exhausted(lex, world):
    od = lm.order(world["words"])
    got, first = [], 0
    while True:
        terms, n_out, n_match = gpu_prefix(lex, [b""], 7, first)
        assert n_match[0] == len(od)
        assert (terms[0, n_out[0]:] == 0xA5A5A5A5).all()
        got += terms[0, :n_out[0]].tolist()
        if n_out[0] < 7:
            break
        first += 7
    assert got == od.tolist()


def test_prefix_edges(lex, world):
    prefixes = [b"abc", b"ab", W64, W64 + b"b", W64 + b"bb", b"abcabcabcabcabcabc", b"ab\xff", b"ab\x00", b"\xff", b"\x00", b"a\xff",
                b"\xc3", b"\xc3\xa9", b"c\xc3\xa9", b"pagerank"]
    for first in (0, 2):
        same(gpu_prefix(lex, prefixes, 9, first), model_prefix(world["words"], prefixes, 9, first))
    n_match = int(model_prefix(world["words"], [b"ab"], 1)[2][0])
    assert n_match > 7
    for first in (n_match - 1, n_match, n_match + 5):
        same(gpu_prefix(lex, [b"ab", b"abc"], 7, first), model_prefix(world["words"], [b"ab", b"abc"], 7, first))
    got = gpu_prefix(lex, prefixes, 9, 0, with_match=False)
    assert got[2] is None
    same(got, model_prefix(world["words"], prefixes, 9, 0)[:2])


# ---- 3. suggest: chunk seams
def test_chunk_seams_inside_a_length_group(ss_ctx):
    """33 words of length 5 between groups of length 4 and 6: a chunk of 32, 33 and 34 words puts the group at chunk + 1, chunk and
    chunk - 1; 1 and 7 make many chunks.  The same bytes for every setting and for the default."""
    words = [w for w in random_words(4000, seed=21, max_len=6) if len(w) in (4, 6)][:50]
    words += [w for w in random_words(4000, seed=22, max_len=5) if len(w) == 5][:33]
    assert sum(len(w) == 5 for w in words) == 33
    freq = (np.arange(len(words)) % 4).astype(np.uint32)
    queries = [words[60], words[82], b"abcab", b"\xc3\xa9abc", b"abca", b"cabcab"]
    lx = engine.Lexicon(ss_ctx, words, freq)
    try:
        for max_dist, m in ((0, 5), (1, 5), (2, 64)):
            want = model_suggest(words, freq, queries, max_dist, m, 0)
            same(gpu_suggest(lx, queries, max_dist, m, 0), want)
            for chunk in (32, 33, 34, 1, 7):
                ss_ctx.set_option("lexicon.chunk_terms", chunk)
                same(gpu_suggest(lx, queries, max_dist, m, 0), want)
            ss_ctx.set_option("lexicon.chunk_terms", None)
    finally:
        ss_ctx.set_option("lexicon.chunk_terms", None)
        lx.close()


@pytest.mark.parametrize("m", [1, 5, 64])
def test_more_candidates_than_m_in_one_chunk_and_over_many(ss_ctx, lex, world, m):
    queries = [b"a", b"abc", b"\xc3\xa9", b"cab"]
    want = ref_suggest(world, queries, 2, m, 0)
    assert (want[2] == m).all()                           # every row is cut at m
    same(gpu_suggest(lex, queries, 2, m, 0), want)        # the default: a range is one chunk
    ss_ctx.set_option("lexicon.chunk_terms", 16)          # ... and dozens of them
    same(gpu_suggest(lex, queries, 2, m, 0), want)


# ---- 4. suggest: values
@pytest.mark.parametrize("max_dist", [0, 1, 2, 3])
def test_suggest_values(lex, world, max_dist):
    queries = [b"", b"a", W64, W64 + b"b", W64[:63] + b"c", b"bacab" + W64[5:], W64[:62] + b"ac", W64[1:], b"pagernak", b"pagerank",
               b"pgaerank", b"abcab\xc3", b"\xa9\xc3", b"abccbaabccba", b"cccccccccccc"]
    want = ref_suggest(world, queries, max_dist, 10, 1)
    same(gpu_suggest(lex, queries, max_dist, 10, 1), want)


def test_one_byte_query_at_distance_three(lex, world):
    want = ref_suggest(world, [b"b", b""], 3, 64, 0)
    assert (want[2] == 64).all()
    same(gpu_suggest(lex, [b"b", b""], 3, 64, 0), want)


def test_min_freq_above_every_freq_gives_empty_rows(lex, world):
    got = gpu_suggest(lex, [b"abc", b"pagerank"], 2, 5, int(world["freq"].max()) + 1)
    assert got[2].tolist() == [0, 0]
    assert got[0].tobytes() == bytes([FILL]) * got[0].nbytes and got[1].tobytes() == bytes([FILL]) * got[1].nbytes


def test_set_freq_reorders_a_row_and_dist_out_may_be_null(lex, world):
    queries = [b"pagerank", b"abc"]
    before = ref_suggest(world, queries, 1, 6, 0)
    same(gpu_suggest(lex, queries, 1, 6, 0), before)
    freq = world["freq"].copy()
    freq[world["words"].index(b"pagerakn")] = 1000        # the swapped word now leads distance 1
    freq[len(world["words"]) - len(HAND) + 3] = 77        # the last "abc" now leads distance 0
    lex.set_freq(freq)
    after = ref_suggest(world, queries, 1, 6, 0, freq)
    assert after[0].tobytes() != before[0].tobytes()
    got = gpu_suggest(lex, queries, 1, 6, 0, with_dist=False)
    assert got[1] is None
    same(got, (after[0], None, after[2]))
    lex.set_freq(None)                                    # all 0: by distance, then id
    same(gpu_suggest(lex, queries, 1, 6, 0), ref_suggest(world, queries, 1, 6, 0, np.zeros_like(freq)))


# ---- 5. device-only chain
def test_device_chain_over_more_rounds_than_turns(ss_ctx, lex, world):
    """suggest -> prefix with every output in device memory, four rounds back to back (more than the lexicon has turns), alternating
    two batches, nothing waited for until the one synchronise at the end; then the same rows through host buffers"""
    import torch
    lib = ss_ctx.lib
    m, k = 5, 7
    batches = [([b"pagernak", b"abd", b""], [b"ab", b"", b"\xc3\xa9c"]), ([b"cabcab\xa9", b"a"], [b"pager", b"c"])]
    rounds = []
    for r in range(4):
        qs, ps = batches[r % 2]
        w_ptr, w_bytes = lm.flatten32(qs)
        p_ptr, p_bytes = lm.flatten32(ps)
        dev = lambda n, itemsize: torch.full((n * itemsize,), FILL, dtype=torch.uint8, device="cuda")   # noqa: E731
        rounds.append({"qs": qs, "ps": ps, "w": (w_ptr, w_bytes), "p": (p_ptr, p_bytes),
                       "st": dev(len(qs) * m, 4), "sd": dev(len(qs) * m, 4), "sn": dev(len(qs), 4),
                       "pt": dev(len(ps) * k, 4), "pn": dev(len(ps), 4), "pm": dev(len(ps), 8)})
    torch.cuda.synchronize()
    for c in rounds:
        assert lib.ss_lexicon_suggest(lex.h, len(c["qs"]), c["w"][0].ctypes.data, c["w"][1].ctypes.data, 2, 0, m, c["st"].data_ptr(),
                                      c["sd"].data_ptr(), c["sn"].data_ptr()) == 0
        assert lib.ss_lexicon_prefix(lex.h, len(c["ps"]), c["p"][0].ctypes.data, c["p"][1].ctypes.data, 1, k, c["pt"].data_ptr(),
                                     c["pn"].data_ptr(), c["pm"].data_ptr()) == 0
    ss_ctx.synchronize()
    for c in rounds:
        host_s = gpu_suggest(lex, c["qs"], 2, m, 0)
        host_p = gpu_prefix(lex, c["ps"], k, 1)
        same(host_s, ref_suggest(world, c["qs"], 2, m, 0))
        same(host_p, model_prefix(world["words"], c["ps"], k, 1))
        for dev_buf, host in ((c["st"], host_s[0]), (c["sd"], host_s[1]), (c["sn"], host_s[2]), (c["pt"], host_p[0]), (c["pn"], host_p[1]),
                              (c["pm"], host_p[2])):
            assert dev_buf.cpu().numpy().tobytes() == host.tobytes()


# ---- 6. refusals
def test_every_refusal_leaves_the_outputs_untouched(ss_ctx, lex):
    lib = ss_ctx.lib
    ptr, data = lm.flatten32([b"abc", b"ab"])
    bad_ptr = np.array([0, 3, 2], np.uint32)
    terms, dist, n_out, n_match = filled((2, 4), np.uint32), filled((2, 4), np.int32), filled((2,), np.int32), filled((2,), np.uint64)
    P = lambda a: None if a is None else a.ctypes.data                                   # noqa: E731

    def prefix(h=lex.h, n_q=2, p=ptr, first=0, k=4, t=terms, n=n_out):
        return lib.ss_lexicon_prefix(h, n_q, P(p), P(data), first, k, P(t), P(n), P(n_match))

    def suggest(h=lex.h, n_q=2, p=ptr, max_dist=1, m=4, t=terms, n=n_out):
        return lib.ss_lexicon_suggest(h, n_q, P(p), P(data), max_dist, 0, m, P(t), P(dist), P(n))

    for call in (prefix, suggest):
        assert call(h=None) == ERR_INVALID
        assert call(t=None) == ERR_INVALID
        assert call(n=None) == ERR_INVALID
        assert call(p=None) == ERR_INVALID
        assert call(n_q=-1) == ERR_INVALID
        assert call(p=bad_ptr) == ERR_INVALID
    assert prefix(k=0) == ERR_INVALID
    assert prefix(first=-1) == ERR_INVALID
    assert prefix(k=lm_max_topk() + 1) == ERR_UNSUPPORTED
    assert suggest(m=0) == ERR_INVALID
    assert suggest(max_dist=-1) == ERR_INVALID
    assert suggest(m=lm.MAX_SUGGEST + 1) == ERR_UNSUPPORTED
    assert suggest(max_dist=lm.MAX_EDIT_DIST + 1) == ERR_UNSUPPORTED
    assert prefix(n_q=0) == 0 and suggest(n_q=0) == 0     # SS_OK, and nothing is done
    for a in (terms, dist, n_out, n_match):
        assert a.tobytes() == bytes([FILL]) * a.nbytes
    # create: word_ptr must start at 0 and never decrease
    for wp in (np.array([1, 2, 3], np.uint64), np.array([0, 3, 2], np.uint64)):
        h = C.c_void_p()
        assert lib.ss_lexicon_create(ss_ctx.h, 2, wp.ctypes.data, data.ctypes.data, None, C.byref(h)) == ERR_INVALID and not h.value
    with pytest.raises(SpaghettiError):
        lex.suggest([b"abc"], max_dist=4)
    assert lib.ss_lexicon_read_order(lex.h, None) == ERR_INVALID and lib.ss_lexicon_destroy(None) == ERR_INVALID


def lm_max_topk():
    from spaghettisearch_amd import _lib
    return _lib.SS_MAX_TOPK
