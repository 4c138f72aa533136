"""GPU parity: word completions (ss_lexicon_complete) vs the Python model (tests/lexicon_complete_model.py).  Every comparison is
tobytes() on whole output arrays that start from 0xA5 bytes, so an entry the call must not write is checked with the ones it must.
The vocabularies are about 4000 random words of length 0 .. 12 over the alphabet a b c 0xC3 0xA9 plus hand-placed words, as in
tests/test_gpu_lexicon.py.
"""
import numpy as np
import pytest

from spaghettisearch_amd import engine
from tests import lexicon_complete_model as cm
from tests import lexicon_model as lm
from tests.test_gpu_lexicon import FILL, HAND, W64, filled, gpu_prefix, gpu_suggest, model_prefix, model_suggest, same
from tests.test_lexicon_cpu import random_words

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = 1, 7
PARTS = (None, 1, 2, 7, 256)                              # "lexicon.complete_parts": the default and the forced values
R64 = [b"r64" + bytes([97 + i // 26, 97 + i % 26]) for i in range(64)]       # a range of exactly 64 positions under "r64"
R65 = [b"r65" + bytes([97 + i // 26, 97 + i % 26]) for i in range(65)]       # ... and of 65 under "r65"


def gpu_complete(lx, prefixes, m, min_freq=1, with_freq=True, with_match=True):
    n_q = len(prefixes)
    out = (filled((n_q, m), np.uint32), filled((n_q, m), np.uint32) if with_freq else None, filled((n_q,), np.int32),
           filled((n_q,), np.uint64) if with_match else None)
    return lx.complete(prefixes, m, min_freq, out=out)


ORDERS = {}                                               # the model's order of a vocabulary, computed once


def model_complete(words, freq, prefixes, m, min_freq=1):
    n_q = len(prefixes)
    if id(words) not in ORDERS:
        ORDERS[id(words)] = (words, lm.order(words))
    return cm.complete(words, freq, prefixes, min_freq, m, filled((n_q, m), np.uint32), filled((n_q, m), np.uint32), filled((n_q,), np.int32),
                       filled((n_q,), np.uint64), od=ORDERS[id(words)][1])


@pytest.fixture(scope="module")
def world():
    """4000 random words, the 64- and 65-word ranges and the hand-placed words; a Zipf-like freq with many ties and zeros, and both
    ends of the uint32 range (the edge of ~freq) inside the ranges the tests ask for"""
    words = random_words(4000, seed=11) + R64 + R65 + HAND
    rng = np.random.default_rng(12)
    freq = (rng.zipf(1.5, len(words)) % 50).astype(np.uint32)
    od = lm.order(words)
    ab = [int(t) for t in od if words[t][:2] == b"ab"]
    freq[ab[1]], freq[ab[5]], freq[ab[-1]], freq[ab[-2]] = 0xFFFFFFFF, 0, 0xFFFFFFFF, 0xFFFFFFFE
    freq[words.index(R64[0])], freq[words.index(R64[63])], freq[words.index(R65[64])] = 0, 0xFFFFFFFF, 0xFFFFFFFF
    return {"words": words, "freq": freq, "od": od}


@pytest.fixture()
def lex(ss_ctx, world):
    lx = engine.Lexicon(ss_ctx, world["words"], world["freq"])
    yield lx
    lx.close()
    ss_ctx.set_option("lexicon.complete_parts", None)


def for_every_parts(ss_ctx, lx, prefixes, m, min_freq, want):
    for parts in PARTS:
        ss_ctx.set_option("lexicon.complete_parts", parts)
        same(gpu_complete(lx, prefixes, m, min_freq), want)
    ss_ctx.set_option("lexicon.complete_parts", None)


# ---- 1. frequency edge values
@pytest.mark.parametrize("value", [0, 3, 0xFFFFFFFF])
def test_all_freq_equal_is_the_page_of_prefix(ss_ctx, world, value):
    """the cross-check between the two calls: with every freq equal the order is the sort order"""
    lx = engine.Lexicon(ss_ctx, world["words"], np.full(len(world["words"]), value, np.uint32))
    prefixes = [b"", b"a", b"ab", b"abc", b"r64", b"r65", b"\xc3\xa9", b"pagera", b"zz"]
    try:
        for m in (1, 5, 64):
            terms, freq, n_out, n_match = gpu_complete(lx, prefixes, m, 0)
            p_terms, p_n, p_match = gpu_prefix(lx, prefixes, m, 0)
            assert terms.tobytes() == p_terms.tobytes() and n_out.tobytes() == p_n.tobytes() and n_match.tobytes() == p_match.tobytes()
            assert (freq[terms != 0xA5A5A5A5] == value).all()
    finally:
        lx.close()


@pytest.mark.parametrize("m", [1, 5, 64])
def test_freq_zero_and_all_ones_together(ss_ctx, lex, world, m):
    prefixes = [b"ab", b"r64", b"r65", b"", b"a"]
    for min_freq in (0, 1, 0xFFFFFFFF):
        want = model_complete(world["words"], world["freq"], prefixes, m, min_freq)
        if m == 64 and min_freq == 0:
            assert 0 in want[1][1, :want[2][1]] and 0xFFFFFFFF in want[1][1, :want[2][1]]      # "r64": both edges in one row
        for_every_parts(ss_ctx, lex, prefixes, m, min_freq, want)


# ---- 2. parts
@pytest.mark.parametrize("m", [1, 5, 64])
def test_parts_against_the_default(ss_ctx, lex, world, m):
    """a range shorter than P ("pagera": 3 words; "r64" / "r65" under 256 parts), of exactly 64 and of 65 positions, the whole vocabulary,
    and ranges with more than m candidates inside one part ("a", "" under 1, 2 and 7 parts)"""
    prefixes = [b"pagera", b"r64", b"r65", b"", b"a", b"c\xc3", b"abcab"]
    want = model_complete(world["words"], world["freq"], prefixes, m, 1)
    assert want[3].tolist()[:4] == [3, 64, 65, len(world["words"])]
    assert want[2][3] == m and want[2][4] == m
    for_every_parts(ss_ctx, lex, prefixes, m, 1, want)


def test_equal_freq_across_every_seam_and_one_candidate_per_part(ss_ctx, world):
    """under "b" every freq is 7: every part seam of every P lies inside a run of equal freq, and the order is by position alone.  Under
    "c" every freq is 1 but for one word in each of the 7 parts of P = 7, so that min_freq 2 leaves 7 candidates, one per part"""
    words, od = world["words"], world["od"]
    freq = world["freq"].copy()
    b_pos = [pos for pos, t in enumerate(od) if words[t][:1] == b"b"]
    c_pos = [pos for pos, t in enumerate(od) if words[t][:1] == b"c"]
    assert len(b_pos) > 600 and len(c_pos) > 600
    freq[od[b_pos]] = 7
    freq[od[c_pos]] = 1
    lb, n = c_pos[0], len(c_pos)
    for part in range(7):                                 # the middle of part `part` of [lb, lb + n) cut into 7 (lexicon_plan.hpp)
        begin, end = lb + n * part // 7, lb + n * (part + 1) // 7
        freq[od[(begin + end) // 2]] = 1000 - 100 * (part % 3) + part
    lx = engine.Lexicon(ss_ctx, words, freq)
    try:
        for m, min_freq in ((5, 1), (64, 1), (7, 2), (64, 2), (1, 2)):
            want = model_complete(words, freq, [b"b", b"c", b""], m, min_freq)
            if min_freq == 2:
                assert want[2][1] == min(m, 7)
            for_every_parts(ss_ctx, lx, [b"b", b"c", b""], m, min_freq, want)
    finally:
        lx.close()
        ss_ctx.set_option("lexicon.complete_parts", None)


# ---- 3. min_freq
def test_min_freq_above_every_freq_and_cutting_a_row_short(ss_ctx, lex, world):
    prefixes = [b"abc", b"pagerank", b"c", b""]
    got = gpu_complete(lex, prefixes, 5, 0xFFFFFFFF)      # "abc" and "pagerank" hold no word of that freq: empty rows, n_match as ever
    want = model_complete(world["words"], world["freq"], prefixes, 5, 0xFFFFFFFF)
    assert want[2].tolist()[:2] == [0, 0] and (want[3] > 0).all()
    same(got, want)
    assert got[0][:2].tobytes() == bytes([FILL]) * got[0][:2].nbytes and got[1][:2].tobytes() == bytes([FILL]) * got[1][:2].nbytes
    want = model_complete(world["words"], world["freq"], prefixes, 64, 47)
    assert all(0 < n < 64 for n in want[2].tolist()[2:])  # cut short by min_freq, not by m
    for_every_parts(ss_ctx, lex, prefixes, 64, 47, want)


# ---- 4. prefix shapes
def test_prefix_shapes(ss_ctx, lex, world):
    """a prefix equal to a word, longer than every word, matching nothing, ending in 0xFF and in 0x00"""
    prefixes = [b"abc", W64, W64 + b"b", W64 + b"bb", b"zzz", b"ab\xff", b"ab\x00", b"\xff", b"\x00", b"a\xff", b"\xc3", b"\xc3\xa9",
                b"pagerank", b"abcabcabcabcabcabc"]
    for m, min_freq in ((5, 0), (64, 1)):
        for_every_parts(ss_ctx, lex, prefixes, m, min_freq, model_complete(world["words"], world["freq"], prefixes, m, min_freq))


# ---- 5. vocabulary shapes
@pytest.mark.parametrize("words", [[], [b"solo"], [b""], [b"same"] * 70, [b"x" * 70, b"x" * 71]],
                         ids=["none", "one", "one-empty", "duplicates", "longer-than-64"])
def test_tiny_vocabularies(ss_ctx, words):
    freq = (np.arange(len(words)) % 3).astype(np.uint32)  # duplicates with different ids and freq: by freq, then by id
    lx = engine.Lexicon(ss_ctx, words, freq)
    prefixes = [b"", b"s", b"same", b"solo", b"t", b"x" * 70]
    try:
        for m, min_freq in ((7, 0), (64, 1), (1, 0)):
            for_every_parts(ss_ctx, lx, prefixes, m, min_freq, model_complete(words, freq, prefixes, m, min_freq))
    finally:
        lx.close()
        ss_ctx.set_option("lexicon.complete_parts", None)


# ---- 6. other paths
def test_set_freq_reorders_a_row_and_nullable_outputs(lex, world):
    prefixes = [b"pager", b"abc"]
    before = model_complete(world["words"], world["freq"], prefixes, 6, 0)
    same(gpu_complete(lex, prefixes, 6, 0), before)
    freq = world["freq"].copy()
    freq[world["words"].index(b"pagerakn")] = 1000        # now leads the "pager" row
    freq[len(world["words"]) - len(HAND) + 3] = 77        # the second "abc" now leads its row
    lex.set_freq(freq)
    after = model_complete(world["words"], freq, prefixes, 6, 0)
    assert after[0].tobytes() != before[0].tobytes()
    got = gpu_complete(lex, prefixes, 6, 0, with_freq=False)
    assert got[1] is None
    same(got, (after[0], None, after[2], after[3]))
    got = gpu_complete(lex, prefixes, 6, 0, with_match=False)
    assert got[3] is None
    same(got, after[:3] + (None,))
    lex.set_freq(None)                                    # all 0: the sort order
    same(gpu_complete(lex, prefixes, 6, 0), model_complete(world["words"], np.zeros_like(freq), prefixes, 6, 0))


def test_device_chain_over_more_rounds_than_turns(ss_ctx, lex, world):
    """complete -> prefix -> suggest with every output in device memory, four rounds back to back (more than the lexicon has turns),
    alternating two batches, nothing waited for until the one synchronise at the end; then the same rows through host buffers"""
    import torch
    lib = ss_ctx.lib
    m, k = 5, 7
    batches = [([b"pager", b"ab", b""], [b"ab", b"", b"\xc3\xa9c"], [b"pagernak", b"abd"]), ([b"c", b"r65"], [b"pager", b"c"], [b"a"])]
    rounds = []
    for r in range(4):
        cs, ps, qs = batches[r % 2]
        dev = lambda n, itemsize: torch.full((n * itemsize,), FILL, dtype=torch.uint8, device="cuda")   # noqa: E731
        rounds.append({"cs": cs, "ps": ps, "qs": qs, "c": lm.flatten32(cs), "p": lm.flatten32(ps), "w": lm.flatten32(qs),
                       "ct": dev(len(cs) * m, 4), "cf": dev(len(cs) * m, 4), "cn": dev(len(cs), 4), "cm": dev(len(cs), 8),
                       "pt": dev(len(ps) * k, 4), "pn": dev(len(ps), 4), "pm": dev(len(ps), 8),
                       "st": dev(len(qs) * m, 4), "sd": dev(len(qs) * m, 4), "sn": dev(len(qs), 4)})
    torch.cuda.synchronize()
    for c in rounds:
        assert lib.ss_lexicon_complete(lex.h, len(c["cs"]), c["c"][0].ctypes.data, c["c"][1].ctypes.data, 1, m, c["ct"].data_ptr(),
                                       c["cf"].data_ptr(), c["cn"].data_ptr(), c["cm"].data_ptr()) == 0
        assert lib.ss_lexicon_prefix(lex.h, len(c["ps"]), c["p"][0].ctypes.data, c["p"][1].ctypes.data, 1, k, c["pt"].data_ptr(),
                                     c["pn"].data_ptr(), c["pm"].data_ptr()) == 0
        assert lib.ss_lexicon_suggest(lex.h, len(c["qs"]), c["w"][0].ctypes.data, c["w"][1].ctypes.data, 2, 0, m, c["st"].data_ptr(),
                                      c["sd"].data_ptr(), c["sn"].data_ptr()) == 0
    ss_ctx.synchronize()
    for c in rounds:
        host_c = gpu_complete(lex, c["cs"], m, 1)
        host_p = gpu_prefix(lex, c["ps"], k, 1)
        host_s = gpu_suggest(lex, c["qs"], 2, m, 0)
        same(host_c, model_complete(world["words"], world["freq"], c["cs"], m, 1))
        same(host_p, model_prefix(world["words"], c["ps"], k, 1))
        same(host_s, model_suggest(world["words"], world["freq"], c["qs"], 2, m, 0))
        for dev_buf, host in ((c["ct"], host_c[0]), (c["cf"], host_c[1]), (c["cn"], host_c[2]), (c["cm"], host_c[3]), (c["pt"], host_p[0]),
                              (c["pn"], host_p[1]), (c["pm"], host_p[2]), (c["st"], host_s[0]), (c["sd"], host_s[1]), (c["sn"], host_s[2])):
            assert dev_buf.cpu().numpy().tobytes() == host.tobytes()


def test_every_refusal_leaves_the_outputs_untouched(ss_ctx, lex):
    lib = ss_ctx.lib
    ptr, data = lm.flatten32([b"abc", b"ab"])
    bad_ptr = np.array([0, 3, 2], np.uint32)
    terms, freq, n_out, n_match = filled((2, 4), np.uint32), filled((2, 4), np.uint32), filled((2,), np.int32), filled((2,), np.uint64)
    P = lambda a: None if a is None else a.ctypes.data                                   # noqa: E731

    def complete(h=lex.h, n_q=2, p=ptr, d=data, m=4, t=terms, n=n_out):
        return lib.ss_lexicon_complete(h, n_q, P(p), P(d), 0, m, P(t), P(freq), P(n), P(n_match))

    assert complete(h=None) == ERR_INVALID
    assert complete(t=None) == ERR_INVALID
    assert complete(n=None) == ERR_INVALID
    assert complete(p=None) == ERR_INVALID
    assert complete(d=None) == ERR_INVALID
    assert complete(n_q=-1) == ERR_INVALID
    assert complete(p=bad_ptr) == ERR_INVALID
    assert complete(m=0) == ERR_INVALID
    assert complete(m=-3) == ERR_INVALID
    assert complete(m=cm.MAX_COMPLETE + 1) == ERR_UNSUPPORTED
    assert complete(n_q=0) == 0                           # SS_OK, and nothing is done
    for a in (terms, freq, n_out, n_match):
        assert a.tobytes() == bytes([FILL]) * a.nbytes
    assert complete() == 0 and (n_out >= 0).all()                                        # ... and the same arguments pass
