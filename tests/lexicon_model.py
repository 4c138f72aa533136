"""Plain Python / numpy model of the term lexicon (include/spaghetti_rank.h: ss_lexicon_*), written straight from the header:
the sort order, the word list by prefix with paging, the optimal-string-alignment distance over bytes and the suggestions.
Words are `bytes` objects; word t is words[t]."""
from __future__ import annotations

import numpy as np

MAX_WORD_BYTES = 64
MAX_EDIT_DIST = 3
MAX_SUGGEST = 64


def flatten(words):
    """-> (ptr uint64 [n + 1], bytes uint8): the arrays ss_lexicon_create takes"""
    ptr = np.zeros(len(words) + 1, dtype=np.uint64)
    if words:
        ptr[1:] = np.cumsum([len(w) for w in words], dtype=np.uint64)
    data = np.frombuffer(b"".join(words), dtype=np.uint8).copy()
    return ptr, data


def flatten32(words):
    """-> (ptr uint32 [n + 1], bytes uint8): the arrays of a call (p_ptr / w_ptr)"""
    ptr, data = flatten(words)
    return ptr.astype(np.uint32), data


def _before(a: bytes, ia: int, b: bytes, ib: int) -> bool:
    """unsigned bytes, lexicographically, a proper prefix first; equal words by id"""
    n = min(len(a), len(b))
    for i in range(n):
        if a[i] != b[i]:
            return a[i] < b[i]          # (indexing bytes gives 0 .. 255: unsigned)
    if len(a) != len(b):
        return len(a) < len(b)
    return ia < ib


def order(words) -> np.ndarray:
    """the permutation that sorts the words (merge sort on the comparison above: no reliance on Python's own bytes ordering)"""
    def sort(ids):
        if len(ids) <= 1:
            return ids
        mid = len(ids) // 2
        a, b = sort(ids[:mid]), sort(ids[mid:])
        out, i, j = [], 0, 0
        while i < len(a) and j < len(b):
            if _before(words[b[j]], b[j], words[a[i]], a[i]):
                out.append(b[j])
                j += 1
            else:
                out.append(a[i])
                i += 1
        return out + a[i:] + b[j:]
    return np.array(sort(list(range(len(words)))), dtype=np.uint32)


def prefix(words, prefixes, first: int, k: int, terms=None, n_out=None, n_match=None, od=None):
    """-> (terms uint32 [n_q][k], n_out int32 [n_q], n_match uint64 [n_q]); entries past n_out[q] keep what `terms` held.
    od: order(words), if the caller has it already"""
    n_q = len(prefixes)
    terms = np.zeros((n_q, k), dtype=np.uint32) if terms is None else terms
    n_out = np.zeros(n_q, dtype=np.int32) if n_out is None else n_out
    n_match = np.zeros(n_q, dtype=np.uint64) if n_match is None else n_match
    od = order(words) if od is None else od
    for q, pre in enumerate(prefixes):
        match = [int(t) for t in od if words[t][:len(pre)] == pre]
        n_match[q] = len(match)
        n = min(max(len(match) - first, 0), k)
        n_out[q] = n
        terms[q, :n] = match[first:first + n]
    return terms, n_out, n_match


def osa(a: bytes, b: bytes) -> int:
    """the recurrence of the header, two rows back for the swap of adjacent bytes"""
    la, lb = len(a), len(b)
    prev2 = None
    prev = list(range(lb + 1))
    for i in range(1, la + 1):
        cur = [i] + [0] * lb
        for j in range(1, lb + 1):
            v = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (a[i - 1] != b[j - 1]))
            if i >= 2 and j >= 2 and a[i - 1] == b[j - 2] and a[i - 2] == b[j - 1]:
                v = min(v, prev2[j - 2] + 1)
            cur[j] = v
        prev2, prev = prev, cur
    return prev[lb]


def suggest(words, freq, queries, max_dist: int, min_freq: int, m: int, terms=None, dist=None, n_out=None):
    """-> (terms uint32 [n_q][m], dist int32 [n_q][m], n_out int32 [n_q]); entries past n_out[q] keep what the arrays held"""
    n_q = len(queries)
    terms = np.zeros((n_q, m), dtype=np.uint32) if terms is None else terms
    dist = np.zeros((n_q, m), dtype=np.int32) if dist is None else dist
    n_out = np.zeros(n_q, dtype=np.int32) if n_out is None else n_out
    freq = np.zeros(len(words), dtype=np.uint32) if freq is None else freq
    for q, w in enumerate(queries):
        cand = []
        if len(w) <= MAX_WORD_BYTES:
            for t, x in enumerate(words):
                if len(x) > MAX_WORD_BYTES or int(freq[t]) < min_freq or abs(len(x) - len(w)) > max_dist:
                    continue                      # (a length difference is a lower bound of the distance)
                d = osa(w, x)
                if d <= max_dist:
                    cand.append((d, -int(freq[t]), t))
        cand.sort()
        n = min(m, len(cand))
        n_out[q] = n
        for r in range(n):
            terms[q, r] = cand[r][2]
            dist[q, r] = cand[r][0]
    return terms, dist, n_out
