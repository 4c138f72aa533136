"""CPU checks of the completions' model (tests/lexicon_complete_model.py) against an independent brute-force restatement — sorted()
over all words with (-freq, word, id) as the key, no sort order and no 64-bit key — and the hand cases of include/spaghetti_rank.h
("Complete").  The GPU tests compare the library with the model; this file is what makes the model trustworthy."""
import numpy as np
import pytest

from tests import lexicon_complete_model as cm
from tests.test_lexicon_cpu import random_words

FILL = 0xA5


def filled(shape, dtype):
    return np.frombuffer(bytes([FILL]) * (int(np.prod(shape)) * np.dtype(dtype).itemsize), dtype=dtype).reshape(shape).copy()


def brute(words, freq, pre, min_freq, m):
    """-> (rows [(term, freq)], n_match): Python compares bytes as unsigned, a proper prefix first"""
    match = [t for t, w in enumerate(words) if w.startswith(pre)]
    cand = sorted((-int(freq[t]), words[t], t) for t in match if int(freq[t]) >= min_freq)
    return [(t, -f) for f, _, t in cand[:m]], len(match)


HAND_WORDS = [b"car", b"cat", b"ca", b"dog", b"cat", b"cab"]
HAND_FREQ = np.array([5, 9, 5, 100, 9, 0], dtype=np.uint32)


@pytest.mark.parametrize("pre,min_freq,m,ids,freqs,n_match", [
    (b"ca", 1, 3, [1, 4, 2], [9, 9, 5], 5),
    (b"ca", 1, 64, [1, 4, 2, 0], [9, 9, 5, 5], 5),
    (b"ca", 0, 64, [1, 4, 2, 0, 5], [9, 9, 5, 5, 0], 5),
    (b"ca", 10, 3, [], [], 5),
    (b"", 1, 1, [3], [100], 6),
    (b"cow", 1, 3, [], [], 0),
])
def test_hand_cases_of_the_header(pre, min_freq, m, ids, freqs, n_match):
    terms, freq, n_out, nm = cm.complete(HAND_WORDS, HAND_FREQ, [pre], min_freq, m, filled((1, m), np.uint32), filled((1, m), np.uint32),
                                         filled((1,), np.int32), filled((1,), np.uint64))
    assert n_out.tolist() == [len(ids)] and nm.tolist() == [n_match]
    assert terms[0, :len(ids)].tolist() == ids and freq[0, :len(ids)].tolist() == freqs
    assert (terms[0, len(ids):] == 0xA5A5A5A5).all() and (freq[0, len(ids):] == 0xA5A5A5A5).all()      # left untouched


def test_equal_freq_gives_the_row_of_prefix():
    from tests import lexicon_model as lm
    words = random_words(300, seed=5) + [b"abc", b"abc"]
    prefixes = [b"", b"a", b"ab", b"abc", b"\xc3", b"zz"]
    for value in (0, 7, 0xFFFFFFFF):
        got = cm.complete(words, np.full(len(words), value, np.uint32), prefixes, 0, 9)
        want = lm.prefix(words, prefixes, 0, 9)
        assert got[0].tobytes() == want[0].tobytes() and got[2].tobytes() == want[1].tobytes() and got[3].tobytes() == want[2].tobytes()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_model_against_brute_force(seed):
    words = random_words(500, seed=seed, max_len=6) + [b"abc", b"abc", b"ab\xff", b"ab\x00", b"ab", b""]
    rng = np.random.default_rng(seed + 100)
    freq = (rng.zipf(1.5, len(words)) % 7).astype(np.uint32)                 # many ties and zeros
    freq[:4] = [0xFFFFFFFF, 0, 0xFFFFFFFE, 0xFFFFFFFF]                        # the edge of ~freq
    prefixes = [b"", b"a", b"ab", b"abc", b"abca", b"\xc3", b"\xc3\xa9", b"ab\xff", b"ab\x00", b"\xff", b"cccccccccc"]
    for min_freq, m in ((0, 1), (1, 5), (3, 64), (0xFFFFFFFF, 5), (0, 64)):
        terms, fr, n_out, n_match = cm.complete(words, freq, prefixes, min_freq, m)
        for q, pre in enumerate(prefixes):
            rows, nm = brute(words, freq, pre, min_freq, m)
            assert n_match[q] == nm and n_out[q] == len(rows)
            assert list(zip(terms[q, :n_out[q]].tolist(), fr[q, :n_out[q]].tolist())) == rows
