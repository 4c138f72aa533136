"""The numpy restatement of the token-vector definitions in include/spaghetti_rank.h (ss_hit_maxsim_scores, ss_rerank_hits_by_maxsim):
per query token the largest dot product over a doc's tokens, summed over the query's tokens; int64 inside, asserted to fit int32.
Outputs are written into the arrays given, only where the definitions write."""
import numpy as np

NO_SCORE = -(2 ** 31)            # SS_NO_VEC_SCORE
MAX_QUERY_TOKENS = 64            # SS_MAX_QUERY_TOKENS
MAX_DIM = 1024                   # SS_MAX_VEC_DIM


def maxsim(qrows, drows):
    """the score of one (query, doc): qrows int8 [m][dim], drows int8 [T][dim], T >= 1 -> Python int; m == 0 gives 0"""
    qrows, drows = np.asarray(qrows, np.int8).astype(np.int64), np.asarray(drows, np.int8).astype(np.int64)
    assert drows.shape[0] >= 1
    if qrows.shape[0] == 0:
        return 0
    s = int((qrows @ drows.T).max(axis=1).sum())
    assert -(2 ** 31) < s <= 2 ** 30                            # |maxsim| <= 64 * 2^24, never NO_SCORE
    return s


def window_scores(qt_ptr, qtok, tok_ptr, tok, docs, q):
    """int64 scores of the docs of one window under query q, NO_SCORE for doc >= n_docs or a doc without tokens"""
    n_docs = len(tok_ptr) - 1
    qrows = np.asarray(qtok)[int(qt_ptr[q]):int(qt_ptr[q + 1])]
    cache, out = {}, []
    for d in docs:
        d = int(d)
        if d not in cache:
            if d >= n_docs or int(tok_ptr[d + 1]) == int(tok_ptr[d]):
                cache[d] = NO_SCORE
            else:
                cache[d] = maxsim(qrows, np.asarray(tok)[int(tok_ptr[d]):int(tok_ptr[d + 1])])
        out.append(cache[d])
    return np.array(out, np.int64)


def hit_scores(qt_ptr, qtok, tok_ptr, tok, hits, n_hits, out, clamp=False):
    """out int32 [n_q][k_in]: rows j < n_hits[q] written"""
    k_in = hits.shape[1]
    for q in range(hits.shape[0]):
        n = int(n_hits[q])
        if clamp:
            n = min(max(n, 0), k_in)
        out[q, :n] = window_scores(qt_ptr, qtok, tok_ptr, tok, hits["doc"][q, :n], q)
    return out


def rerank(qt_ptr, qtok, tok_ptr, tok, hits, n_hits, first, k, hits_out, n_out, scores_out=None, clamp=False):
    """the window sorted stably by score descending, rows without a score last in window order; page [first, first + k)"""
    k_in = hits.shape[1]
    for q in range(hits.shape[0]):
        n = int(n_hits[q])
        if clamp:
            n = min(max(n, 0), k_in)
        sc = window_scores(qt_ptr, qtok, tok_ptr, tok, hits["doc"][q, :n], q)
        order = sorted(range(n), key=lambda j: (0, -int(sc[j]), j) if sc[j] != NO_SCORE else (1, 0, j))[first:first + k]
        n_out[q] = len(order)
        for r, j in enumerate(order):
            hits_out[q, r] = hits[q, j]
            if scores_out is not None:
                scores_out[q, r] = sc[j]
    return hits_out, n_out, scores_out


def known_world():
    """the header's known answer: (tok_ptr, tok, qt_ptr, qtok) at dim 64; docs A, B, C (no token), D"""
    docs = [[(10, 0), (0, 3)], [(4, 4)], [], [(-5, -5), (-1, -9)]]
    tok_ptr = np.zeros(5, np.uint64)
    tok_ptr[1:] = np.cumsum([len(d) for d in docs])
    tok = np.zeros((int(tok_ptr[-1]), 64), np.int8)
    tok[:, :2] = [t for d in docs for t in d]
    qtok = np.zeros((2, 64), np.int8)
    qtok[:, :2] = [(1, 0), (0, 2)]
    return tok_ptr, tok, np.array([0, 2], np.uint32), qtok
