"""The definitions of ss_index_build_signatures and ss_dedup_hits (include/spaghetti_rank.h) restated in numpy: the hash, a doc's
signature from its row of the doc view, and the walk over a window as one plain loop over j.  No GPU, no library call, no tiles."""
from __future__ import annotations

import numpy as np

SIG_EMPTY = 0xFFFFFFFF
MAX_SIG_SLOTS = 32

HIT_DTYPE = np.dtype([("doc", "<u4"), ("_pad", "<u4"), ("title", "<f8"), ("body", "<f8"), ("pagerank", "<f8"), ("final", "<f8")])


def h(t, s):
    """h(t, s) for arrays (or scalars) of term ids and slot numbers, broadcast against each other -> uint32."""
    with np.errstate(over="ignore"):
        x = np.asarray(t, dtype=np.uint32) + np.uint32(0x9E3779B9) * (np.asarray(s, dtype=np.uint32) + np.uint32(1))
        x = x ^ (x >> np.uint32(16))
        x = x * np.uint32(0x85EBCA6B)
        x = x ^ (x >> np.uint32(13))
        x = x * np.uint32(0xC2B2AE35)
        x = x ^ (x >> np.uint32(16))
    return x.astype(np.uint32)


def h_int(t, s):
    """The same with Python integers and explicit masks: a second implementation to check the first."""
    m = 0xFFFFFFFF
    x = (t + 0x9E3779B9 * (s + 1)) & m
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & m
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & m
    x ^= x >> 16
    return x


def row_signature(terms, n_slots):
    """The signature of one term set (any order, duplicates allowed) -> uint32[n_slots]."""
    terms = np.asarray(terms, dtype=np.uint32)
    if terms.size == 0:
        return np.full(n_slots, SIG_EMPTY, dtype=np.uint32)
    return h(terms[:, None], np.arange(n_slots, dtype=np.uint32)[None, :]).min(axis=0).astype(np.uint32)


def signatures(doc_ptr, doc_term, n_slots):
    """sig uint32[n_docs][n_slots] from a doc view (doc_ptr uint64[n_docs+1], doc_term uint32[P])."""
    n_docs = len(doc_ptr) - 1
    sig = np.full((n_docs, n_slots), SIG_EMPTY, dtype=np.uint32)
    slots = np.arange(n_slots, dtype=np.uint32)
    for s in slots:                                   # per slot one pass: hash every posting, minimum per non-empty row
        hv = h(doc_term, s)
        starts = np.asarray(doc_ptr[:-1], dtype=np.int64)
        lens = np.diff(np.asarray(doc_ptr, dtype=np.int64))
        nz = lens > 0
        if hv.size:
            sig[nz, s] = np.minimum.reduceat(hv, starts[nz])
    return sig


def row_sigs(docs, sig):
    """Per window row its signature, or None for a row on its own (doc outside the table, or a signature that is all SIG_EMPTY)."""
    out = []
    for d in docs:
        d = int(d)
        if d < sig.shape[0] and not np.all(sig[d] == SIG_EMPTY):
            out.append(sig[d])
        else:
            out.append(None)
    return out


def match_matrix(docs, sig):
    """match[i][j] = slots in which rows i and j agree; -1 where either row is on its own (such a pair never matches, i == j included)."""
    rs = row_sigs(docs, sig)
    n = len(rs)
    m = np.full((n, n), -1, dtype=np.int64)
    for i in range(n):
        for j in range(n):
            if rs[i] is not None and rs[j] is not None:
                m[i, j] = int(np.sum(rs[i] == rs[j]))
    return m


def walk(match, min_match):
    """The walk on a match matrix (match[i][j] < 0: never a match) -> (kept indices, leader[j], similar[j] = rows led by j)."""
    n = len(match)
    kept, leader = [], [0] * n
    for j in range(n):
        lead = j
        for i in kept:                                # ascending: the first hit is the smallest
            if match[i][j] >= min_match and match[i][j] >= 0:
                lead = i
                break
        leader[j] = lead
        if lead == j:
            kept.append(j)
    similar = [0] * n
    for j in range(n):
        similar[leader[j]] += 1
    return kept, leader, similar


def dedup(hits, n_hits, sig, min_match, first, k, hits_out, n_hits_out, similar_out=None, n_kept_out=None, clamp=False):
    """Writes the outputs the way the call does (entries past n_hits_out[q] untouched) into the arrays given, and returns them.
    hits [n_q][k_in] HIT_DTYPE; clamp: n_hits outside [0, k_in] is clamped (device n_hits), else it is an error."""
    n_q, k_in = hits.shape
    for q in range(n_q):
        n = int(n_hits[q])
        if n < 0 or n > k_in:
            if not clamp:
                raise ValueError("n_hits outside [0, k_in]")
            n = min(max(n, 0), k_in)
        kept, _, similar = walk(fast_match(hits["doc"][q, :n], sig), min_match)
        page = kept[first:first + k]
        for r, j in enumerate(page):
            hits_out[q, r] = hits[q, j]
            if similar_out is not None:
                similar_out[q, r] = similar[j]
        n_hits_out[q] = len(page)
        if n_kept_out is not None:
            n_kept_out[q] = len(kept)
    return hits_out, n_hits_out, similar_out, n_kept_out


def fast_match(docs, sig):
    """match_matrix with numpy broadcasting (the windows of the GPU tests hold up to 1024 rows)."""
    docs = np.asarray(docs, dtype=np.int64)
    n = len(docs)
    inside = docs < sig.shape[0]
    rows = np.full((n, sig.shape[1]), SIG_EMPTY, dtype=np.uint32)
    rows[inside] = sig[docs[inside]]
    own = np.all(rows == SIG_EMPTY, axis=1)
    m = (rows[:, None, :] == rows[None, :, :]).sum(axis=2).astype(np.int64)
    m[own, :] = -1
    m[:, own] = -1
    return m
