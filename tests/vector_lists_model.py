"""The numpy restatement of the vector-list definitions in include/spaghetti_rank.h (ss_vector_topk_probed, ss_vector_assign_lists) and
of engine.train_vector_lists: an int32 matmul and np.lexsort on (id, -score), on top of tests/vector_model.py, which states the order
of the rows.  Outputs are written into the arrays given, only where the definitions write."""
import numpy as np

from tests import vector_model as vm

NO_LIST = 0xFFFFFFFF             # SS_NO_LIST
MAX_LISTS = 65536                # SS_MAX_VEC_LISTS


def probes(qvec, centroids, n_probe):
    """uint32 [n_q][min(n_probe, n_lists)]: the lists by centroid score descending, then list ascending"""
    sc = vm.scores(qvec, centroids)
    n_lists = sc.shape[1]
    p = min(int(n_probe), n_lists)
    out = np.zeros((sc.shape[0], p), np.uint32)
    for q in range(sc.shape[0]):
        out[q] = np.lexsort((np.arange(n_lists), -sc[q].astype(np.int64)))[:p]
    return out


def topk_probed(qvec, vec, centroids, list_of_doc, k, n_probe, hits, n_hits, mask_id=None, masks=None):
    """vm.topk over the docs whose list is among the query's probes (and in its allow-list) -> hits, n_hits, probes"""
    pr = probes(qvec, centroids, n_probe)
    sc = vm.scores(qvec, vec)
    lod = np.asarray(list_of_doc, np.uint32)
    for q in range(sc.shape[0]):
        allowed = np.isin(lod, pr[q])                          # (NO_LIST is no list id: n_lists <= 65536)
        if mask_id is not None and mask_id[q] >= 0:
            allowed &= np.asarray(masks[mask_id[q]], bool)
        docs = np.flatnonzero(allowed)
        s = sc[q, docs]
        order = np.lexsort((docs, -s.astype(np.int64)))[:k]
        n_hits[q] = len(order)
        hits["doc"][q, :len(order)] = docs[order]
        hits["score"][q, :len(order)] = s[order]
    return hits, n_hits, pr


def assign(vec, centroids):
    """(uint32 [n_docs], int32 [n_docs]): per doc the list of the largest centroid score, ties to the lower list, and that score"""
    sc = vm.scores(vec, centroids)
    lists = np.argmax(sc, axis=1)                              # (the first of equal maxima)
    return lists.astype(np.uint32), sc[np.arange(sc.shape[0]), lists].astype(np.int32)


def train(vec, n_lists, iters, seed):
    """engine.train_vector_lists on the host -> (centroids int8 [n_lists][dim], list_of_doc uint32 [n_docs])"""
    vec = np.ascontiguousarray(vec, dtype=np.int8)
    rng = np.random.default_rng(seed)
    centroids = vec[np.sort(rng.choice(vec.shape[0], size=int(n_lists), replace=False))].copy()
    for _ in range(int(iters)):
        lists, _ = assign(vec, centroids)
        for l in range(int(n_lists)):
            members = vec[lists == l]
            if len(members):
                centroids[l] = np.clip(np.rint(members.astype(np.float64).mean(axis=0)), -128, 127).astype(np.int8)
    return centroids, assign(vec, centroids)[0]
