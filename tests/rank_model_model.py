"""The numpy restatement of learned ranking (include/spaghetti_rank.h: ss_rank_model_*, ss_hit_features, ss_rerank_hits_by_model).
float64 throughout, an explicit loop over the trees so that the additions stand in tree order, every product and sum rounded once
(Python and numpy scalars never fuse).  A model here is a dict {n_features, linear (float64 [n_features] | None), base, trees}; a tree is a
TREE_NODE array (feature, left, right, nan_left, value) whose node 0 is the root."""
import numpy as np

TREE_NODE = np.dtype([("feature", "<i4"), ("left", "<u4"), ("right", "<u4"), ("nan_left", "<u4"), ("value", "<f8")])
PROXIMITY = np.dtype([("start", "<f4"), ("end", "<f4"), ("n_present", "<u4"), ("n_occ", "<u4"), ("token_mask", "<u8")])
N_FEATURES = 15
NO_VEC_SCORE = -(1 << 31)
NO_FIELD_VALUE = -(1 << 63)
NAN_BITS = 0x7FF8000000000000
NAN = np.array([NAN_BITS], dtype=np.uint64).view(np.float64)[0]


def split(f, thr, left, right, nan_left=0):
    return (f, left, right, nan_left, thr)


def leaf(v):
    return (-1, 0, 0, 0, v)


def tree(*nodes):
    return np.array(list(nodes), dtype=TREE_NODE)


def model(n_features, trees, linear=None, base=0.0):
    trees = [np.asarray(t, dtype=TREE_NODE) for t in trees]
    return {"n_features": n_features, "trees": trees, "lists": [t.tolist() for t in trees],      # (lists: the same nodes as Python tuples, for speed)
            "linear": None if linear is None else np.asarray(linear, dtype=np.float64), "base": float(base)}


def walk(t, x):
    """the leaf value tree t (an array or its list of tuples) sends row x to"""
    t = t.tolist() if isinstance(t, np.ndarray) else t
    i = 0
    while t[i][0] >= 0:
        f, left, right, nan_left, value = t[i]
        xv = x[f]
        i = left if (bool(nan_left) if xv != xv else xv <= value) else right
    return t[i][4]


def score_row(m, x):
    """Python floats are IEEE float64 and every + and * below is one rounded operation"""
    x = [float(v) for v in x]
    acc = m["base"]
    if m["linear"] is not None:
        for w, xv in zip(m["linear"].tolist(), x):
            if w != 0.0 and xv == xv:
                acc = acc + w * xv
    for t in m["lists"]:
        acc = acc + walk(t, x)
    return NAN if acc != acc else np.float64(acc)


def scores(m, x):
    """[n_rows] float64: a NaN as the quiet NaN 0x7FF8000000000000"""
    x = np.asarray(x, dtype=np.float64).reshape(-1, m["n_features"])
    return np.array([score_row(m, r) for r in x], dtype=np.float64)


def prox_of(e):
    """column 8: ss_rerank_hits_by_proximity's prox of one entry"""
    n = int(e["n_present"])
    sp = np.float64(e["end"]) - np.float64(e["start"])
    gaps = np.float64(n - 1 if n else (1 << 32) - 1)              # (uint32 arithmetic; unused below 2)
    return np.float64(0.0) if n < 2 else gaps / max(sp, gaps)


def features(hits, n_hits, n_docs, prox=None, vec_scores=None, query_len=None, fields=None, fill=None):
    """[n_q][k_in][15] float64.  fields: int64 [n_fields][n_docs] | None.  fill: what the untouched entries hold (default zeros)."""
    n_q, k_in = hits.shape
    out = np.zeros((n_q, k_in, N_FEATURES), dtype=np.float64) if fill is None else np.array(fill, dtype=np.float64).reshape(n_q, k_in, N_FEATURES).copy()
    bits = out.view(np.uint64)
    n_fields = 0 if fields is None else fields.shape[0]
    for q in range(n_q):
        for j in range(min(max(int(n_hits[q]), 0), k_in)):
            row, f = hits[q, j], out[q, j]
            for c, name in enumerate(("title", "body", "pagerank", "final")):
                bits[q, j, c] = row[name].view(np.uint64)          # the bytes as given
            f[4] = np.float64(j)
            f[5] = NAN if query_len is None else np.float64(int(query_len[q]))
            if prox is None:
                f[6:10] = NAN
            else:
                e = prox[q, j]
                f[6] = np.float64(int(e["n_present"]))
                f[7] = np.float64(e["end"]) - np.float64(e["start"])
                f[8] = prox_of(e)
                f[9] = np.float64(int(e["n_occ"]))
            vs = NO_VEC_SCORE if vec_scores is None else int(vec_scores[q, j])
            f[10] = NAN if vs == NO_VEC_SCORE else np.float64(vs)
            d = int(row["doc"])
            for c in range(4):
                v = int(fields[c, d]) if c < n_fields and d < n_docs else NO_FIELD_VALUE
                f[11 + c] = NAN if v == NO_FIELD_VALUE else np.float64(np.int64(v))
    return out


def rerank(m, hits, n_hits, n_docs, first, k, prox=None, vec_scores=None, query_len=None, fields=None, hits_fill=None, scores_fill=None):
    """-> (hits_out [n_q][k], n_hits_out [n_q], scores_out [n_q][k]); entries past n_hits_out[q] keep the fill (default zeros)"""
    n_q, k_in = hits.shape
    feat = features(hits, n_hits, n_docs, prox, vec_scores, query_len, fields)
    o_hits = np.zeros((n_q, k), dtype=hits.dtype) if hits_fill is None else hits_fill.copy()
    o_sc = np.zeros((n_q, k), dtype=np.float64) if scores_fill is None else scores_fill.copy()
    o_n = np.zeros(n_q, dtype=np.int32)
    for q in range(n_q):
        n = min(max(int(n_hits[q]), 0), k_in)
        keyed = []
        for j in range(n):
            if int(hits[q, j]["doc"]) >= n_docs:
                keyed.append((2, 0.0, j, NAN))
                continue
            s = score_row(m, feat[q, j])
            keyed.append((1, 0.0, j, NAN) if np.isnan(s) else (0, -float(s) + 0.0, j, s))    # (-0.0 == 0.0 as sort keys; inf sorts as a number)
        keyed.sort(key=lambda t: t[:3])
        page = keyed[first:first + k]
        o_n[q] = len(page)
        for r, (_, _, j, s) in enumerate(page):
            o_hits[q, r] = hits[q, j]
            o_sc[q, r] = s
    return o_hits, o_n, o_sc


VALUES = np.array([-np.inf, -2.5, -1.0, -0.0, 0.0, 0.5, 1.0, 3.0, 1e16, np.inf])   # thresholds and feature values share them: x == value happens


def random_tree(rng, n_nodes, n_features):
    """A valid tree of exactly n_nodes (odd) nodes: a random leaf is split again and again, its children appended behind every node."""
    assert n_nodes % 2 == 1
    nodes = [leaf(float(rng.normal()))]
    leaves = [0]
    while len(nodes) < n_nodes:
        i = leaves.pop(int(rng.integers(len(leaves))))
        l, r = len(nodes), len(nodes) + 1
        if rng.integers(2):
            l, r = r, l
        nodes[i] = split(int(rng.integers(n_features)), float(rng.choice(VALUES)), l, r, int(rng.integers(2)))
        nodes += [leaf(float(rng.normal())), leaf(float(rng.normal()))]
        leaves += [len(nodes) - 2, len(nodes) - 1]
    return tree(*nodes)


def random_rows(rng, n_rows, n_features, nan_share=0.1):
    x = rng.choice(VALUES, size=(n_rows, n_features))
    x[rng.random((n_rows, n_features)) < nan_share] = np.nan
    return x


def flat(trees):
    """(tree_ptr uint32 [n + 1], nodes TREE_NODE) of a list of trees"""
    ptr = np.zeros(len(trees) + 1, dtype=np.uint32)
    if trees:
        ptr[1:] = np.cumsum([len(t) for t in trees])
    return ptr, (np.concatenate(trees) if trees else np.zeros(0, dtype=TREE_NODE))


def known_answer():
    """the header's known answer -> (model, the feature rows A, B, C [3][15], their scores, the order of the window (A, B, C))"""
    lin = np.zeros(N_FEATURES)
    lin[3] = 2.0
    m = model(N_FEATURES, [tree(split(8, 0.5, 1, 2, 0), leaf(0.0), leaf(1.0)), tree(split(11, 100.0, 1, 2, 1), leaf(0.25), leaf(-0.25))], lin, 0.5)
    x = np.zeros((3, N_FEATURES))
    x[:, 3] = (1.0, 1.5, 1.0)                   # final
    x[:, 8] = (1.0, NAN, 0.25)                  # prox: B has no entry
    x[:, 11] = (50.0, NAN, 200.0)               # field 0: B's is SS_NO_FIELD_VALUE
    return m, x, np.array([3.75, 4.75, 2.25]), [1, 0, 2]
