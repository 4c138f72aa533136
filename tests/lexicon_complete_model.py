"""Plain Python / numpy model of ss_lexicon_complete (include/spaghetti_rank.h, "Complete"), written straight from the header: the
matches of a prefix are a range of the sort order, the candidates those of them with freq >= min_freq, ordered by the 64-bit key
(~freq << 32) | position.  Words are `bytes` objects; word t is words[t].  The order comes from tests/lexicon_model.py."""
from __future__ import annotations

import numpy as np

from tests import lexicon_model as lm

MAX_COMPLETE = 64


def complete(words, freq, prefixes, min_freq: int, m: int, terms=None, freq_out=None, n_out=None, n_match=None, od=None):
    """-> (terms uint32 [n_q][m], freq uint32 [n_q][m], n_out int32 [n_q], n_match uint64 [n_q]); entries past n_out[q] keep what the
    arrays held.  od: lm.order(words), if the caller has it already"""
    n_q = len(prefixes)
    terms = np.zeros((n_q, m), dtype=np.uint32) if terms is None else terms
    freq_out = np.zeros((n_q, m), dtype=np.uint32) if freq_out is None else freq_out
    n_out = np.zeros(n_q, dtype=np.int32) if n_out is None else n_out
    n_match = np.zeros(n_q, dtype=np.uint64) if n_match is None else n_match
    freq = np.zeros(len(words), dtype=np.uint32) if freq is None else freq
    od = lm.order(words) if od is None else od
    for q, pre in enumerate(prefixes):
        match = [pos for pos, t in enumerate(od) if words[t][:len(pre)] == pre]
        assert match == list(range(match[0], match[0] + len(match))) if match else True     # a contiguous range [lb, ub)
        n_match[q] = len(match)
        keys = sorted((((~int(freq[od[pos]])) & 0xFFFFFFFF) << 32) | pos for pos in match if int(freq[od[pos]]) >= min_freq)
        n = min(m, len(keys))
        n_out[q] = n
        for r in range(n):
            terms[q, r] = od[keys[r] & 0xFFFFFFFF]
            freq_out[q, r] = (~(keys[r] >> 32)) & 0xFFFFFFFF
    return terms, freq_out, n_out, n_match
