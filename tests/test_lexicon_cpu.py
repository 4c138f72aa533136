"""CPU checks of the term lexicon's model (tests/lexicon_model.py) against an independent brute-force restatement — the full DP
matrix, sorted() on bytes objects — and the hand cases of include/spaghetti_rank.h.  The GPU tests compare the library with the
model; this file is what makes the model trustworthy."""
import numpy as np
import pytest

from tests import lexicon_model as lm

ALPHABET = [b"a", b"b", b"c", b"\xc3", b"\xa9"]       # near neighbours, duplicates and high bytes are dense


def random_words(n, seed, max_len=12):
    rng = np.random.default_rng(seed)
    return [b"".join(ALPHABET[i] for i in rng.integers(0, len(ALPHABET), rng.integers(0, max_len + 1))) for _ in range(n)]


def osa_matrix(a: bytes, b: bytes) -> int:
    """the header's recurrence on the whole (la + 1) x (lb + 1) matrix"""
    D = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(len(a) + 1):
        D[i][0] = i
    for j in range(len(b) + 1):
        D[0][j] = j
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            best = min(D[i - 1][j] + 1, D[i][j - 1] + 1, D[i - 1][j - 1] + (0 if a[i - 1] == b[j - 1] else 1))
            if i >= 2 and j >= 2 and a[i - 1] == b[j - 2] and a[i - 2] == b[j - 1]:
                best = min(best, D[i - 2][j - 2] + 1)
            D[i][j] = best
    return D[len(a)][len(b)]


def brute_order(words):
    return [t for _, t in sorted((w, t) for t, w in enumerate(words))]     # Python compares bytes as unsigned, a prefix first


def brute_suggest(words, freq, w, max_dist, min_freq, m):
    if len(w) > lm.MAX_WORD_BYTES:
        return []
    cand = [(osa_matrix(w, x), -int(freq[t]), t) for t, x in enumerate(words) if len(x) <= lm.MAX_WORD_BYTES and int(freq[t]) >= min_freq]
    return [(t, d) for d, _, t in sorted(c for c in cand if c[0] <= max_dist)][:m]


# ---- distance
def test_the_two_distances_of_the_header():
    assert lm.osa(b"ab", b"ba") == 1
    assert lm.osa(b"ca", b"abc") == 3          # unrestricted Damerau would say 2


def test_distance_of_a_word_with_itself_and_with_the_empty_word():
    for w in (b"", b"a", b"\xc3\xa9", b"abcabc", b"\x00\x00"):
        assert lm.osa(w, w) == 0
    for n in range(1, 5):
        w = b"abca"[:n]
        assert lm.osa(b"", w) == n and lm.osa(w, b"") == n


def test_distance_counts_bytes_not_code_points():
    assert lm.osa("é".encode(), b"e") == 2     # two bytes against one: a substitution and a deletion
    assert lm.osa("né".encode(), "én".encode()) == 2


def test_distance_equals_the_full_matrix():
    words = random_words(120, seed=1, max_len=9)
    for a in words[:40]:
        for b in words:
            assert lm.osa(a, b) == osa_matrix(a, b) == osa_matrix(b, a), (a, b)


# ---- order
def test_high_bytes_sort_after_ascii():
    words = [b"\xc3\xa9", b"z", b"a\xff", b"ab", b"\x80", b"\x7f"]
    assert lm.order(words).tolist() == [3, 2, 1, 5, 4, 0]      # ab < a\xff < z < \x7f < \x80 < \xc3\xa9: a signed compare fails this


def test_a_proper_prefix_sorts_before_its_extensions():
    words = [b"abc", b"ab", b"", b"a", b"ab\x00"]
    assert lm.order(words).tolist() == [2, 3, 1, 4, 0]


def test_duplicate_words_are_ordered_by_id():
    words = [b"b", b"a", b"b", b"a", b"b"]
    assert lm.order(words).tolist() == [1, 3, 0, 2, 4]


def test_order_equals_sorted():
    for seed, n in ((2, 0), (3, 1), (4, 700)):
        words = random_words(n, seed)
        assert lm.order(words).tolist() == brute_order(words)


# ---- prefix
def test_prefix_pages_equal_sorted():
    words = random_words(500, seed=5) + [b"abc", b"abc", b"ab\xff", b"ab\x00"]
    od = brute_order(words)
    for pre in (b"", b"a", b"ab", b"abc", b"ab\xff", b"ab\x00", b"\xc3", b"abcabcabcabcabc", b"zz"):
        match = [t for t in od if words[t].startswith(pre)]
        for first in (0, 3, max(len(match) - 1, 0), len(match), len(match) + 5):
            terms, n_out, n_match = lm.prefix(words, [pre], first, 7, terms=np.full((1, 7), 0xA5A5A5A5, np.uint32))
            want = match[first:first + 7]
            assert n_match[0] == len(match) and n_out[0] == len(want)
            assert terms[0, :len(want)].tolist() == want and (terms[0, len(want):] == 0xA5A5A5A5).all()


# ---- suggest
def test_suggest_equals_brute_force():
    words = random_words(400, seed=6, max_len=8) + [b"x" * 64, b"x" * 65]
    rng = np.random.default_rng(7)
    freq = rng.integers(0, 6, len(words)).astype(np.uint32)
    queries = random_words(12, seed=8, max_len=8) + [b"", b"a", b"x" * 64, b"x" * 65, b"x" * 63]
    for max_dist in (0, 1, 2, 3):
        for min_freq, m in ((0, 64), (1, 5), (3, 1)):
            terms, dist, n_out = lm.suggest(words, freq, queries, max_dist, min_freq, m)
            for q, w in enumerate(queries):
                want = brute_suggest(words, freq, w, max_dist, min_freq, m)
                assert n_out[q] == len(want)
                assert list(zip(terms[q, :n_out[q]].tolist(), dist[q, :n_out[q]].tolist())) == want, (w, max_dist, min_freq, m)


def test_suggest_tie_chain_distance_then_freq_then_id():
    #        0        1        2        3        4        5        6
    words = [b"abcd", b"abce", b"abcf", b"abdc", b"abcd", b"xbcd", b"abcde"]
    freq = np.array([1, 9, 9, 2, 5, 9, 9], np.uint32)
    terms, dist, n_out = lm.suggest(words, freq, [b"abcd"], 1, 1, 64)
    # distance 0: ids 4 (freq 5) then 0 (freq 1); distance 1: freq 9 by id (1, 2, 5, 6), then the swap (id 3, freq 2)
    assert terms[0, :n_out[0]].tolist() == [4, 0, 1, 2, 5, 6, 3]
    assert dist[0, :n_out[0]].tolist() == [0, 0, 1, 1, 1, 1, 1]


def test_suggest_min_freq_and_long_words():
    words = [b"abc", b"abd", b"y" * 65]
    freq = np.array([3, 7, 100], np.uint32)
    assert lm.suggest(words, freq, [b"abc"], 1, 4, 5)[0][0, :1].tolist() == [1]
    assert lm.suggest(words, freq, [b"abc"], 1, 8, 5)[2].tolist() == [0]
    assert lm.suggest(words, freq, [b"y" * 65, b"y" * 64], 3, 0, 5)[2].tolist() == [0, 0]     # a word of 65 bytes is never a candidate
    assert lm.suggest(words, None, [b"abc"], 0, 0, 5)[0][0, :1].tolist() == [0]               # freq None = all 0


def test_untouched_entries_keep_their_bytes():
    terms = np.full((1, 4), 0xA5A5A5A5, np.uint32)
    dist = np.full((1, 4), -1, np.int32)
    lm.suggest([b"ab", b"zz"], None, [b"ab"], 1, 0, 4, terms=terms, dist=dist)
    assert terms[0].tolist() == [0, 0xA5A5A5A5, 0xA5A5A5A5, 0xA5A5A5A5] and dist[0].tolist() == [0, -1, -1, -1]
