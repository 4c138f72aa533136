"""Query operators at BASELINE config 3's full size (10M docs / 1M terms / 640M+40M postings, inputs generated on the device):
ss_score_topk_constrained against ss_score_topk_masked over the same allowed sets built on the host (whole batch, bytes), and
against the posting-deleted oracle (tests/test_gpu_doc_masks.py) on a sample of the batch."""
import numpy as np
import pytest

from spaghettisearch_amd import engine, synth
from tests.test_gpu_doc_masks import masked_ref
from tests.test_gpu_score import assert_same_hits

pytestmark = pytest.mark.gpu


def test_full_size_config3(ss_ctx, oracle):
    """1024 x 3-term OR queries, k = 100; every other query constrained, in turn: one excluded head term, one required tail term,
    one required term that is also one of its query terms."""
    import torch
    ND, NT, PB, PT = 10_000_000, 1_000_000, 640_000_000, 40_000_000
    dev = torch.device("cuda", 0)
    b_ptr, b_doc, b_tf = synth.zipf_index_torch(ND, NT, PB, seed=44, device=dev)
    t_ptr, t_doc, t_tf = synth.zipf_index_torch(ND, NT, PT, seed=144, device=dev)
    bi = engine.InvertedIndex(ss_ctx, ND, b_ptr, b_doc, b_tf)
    ti = engine.InvertedIndex(ss_ctx, ND, t_ptr, t_doc, t_tf)
    wt, mt, _ = ti.tfidf_build(ND, want_idf=False)
    wb, mb, _ = bi.tfidf_build(ND, want_idf=False)
    sc = engine.Scorer(ss_ctx, ti, bi)
    try:
        nq, k = 1024, 100
        q_ptr, q_terms = synth.make_queries(nq, 3, 10_000, seed=45)
        req, exc = [[] for _ in range(nq)], [[] for _ in range(nq)]
        for q in range(0, nq, 2):
            kind = (q // 2) % 3
            if kind == 0:
                exc[q] = [(q // 6) % 3]                                  # a head term
            elif kind == 1:
                req[q] = [5000 + (q // 6) % 4]                           # a tail term, outside the query
            else:
                req[q] = [int(q_terms[q_ptr[q] + 1])]                    # a term of the query itself
        pack = lambda lists: (np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint32),      # noqa: E731
                              np.array([t for x in lists for t in x], np.uint32))
        hits, n_hits = sc.score_topk_constrained(q_ptr, q_terms, k, req=pack(req), exc=pack(exc))
        plain, pn = sc.score_topk(q_ptr, q_terms, k)
        assert hits[1::2].tobytes() == plain[1::2].tobytes() and n_hits[1::2].tolist() == pn[1::2].tolist()

        h = {"b": (b_ptr.cpu().numpy().view(np.uint64), b_doc.cpu().numpy().view(np.uint32), wb),
             "t": (t_ptr.cpu().numpy().view(np.uint64), t_doc.cpu().numpy().view(np.uint32), wt)}

        def allowed_of(r, e):
            a = np.ones(ND, dtype=bool)
            for terms, want in ((r, True), (e, False)):
                for t in terms:
                    c = np.zeros(ND, dtype=bool)
                    for ptr, doc, _ in h.values():
                        c[doc[int(ptr[t]):int(ptr[t + 1])]] = True
                    a &= c if want else ~c
            return a

        # the same sets registered as allow-lists: ss_score_topk_masked gives the same bytes for the whole batch
        keys, words, mask_id = {}, [], np.full(nq, -1, np.int32)
        for q in range(0, nq, 2):
            key = (tuple(req[q]), tuple(exc[q]))
            if key not in keys:
                keys[key] = len(words)
                words.append(engine.pack_doc_masks(allowed_of(*key)[None, :], ND)[0])
            mask_id[q] = keys[key]
        sc.set_doc_masks(np.stack(words))
        mh, mn = sc.score_topk_masked(q_ptr, q_terms, mask_id, k)
        assert hits.tobytes() == mh.tobytes() and n_hits.tolist() == mn.tolist()
        sc.set_doc_masks(None)
        assert (n_hits[0::2] > 0).mean() > 0.5

        # the oracle on a sample of the batch (the sample's lists only)
        ns = 24
        terms = np.unique(np.concatenate([q_terms[:3 * ns], np.array([t for q in range(ns) for t in req[q] + exc[q]], np.uint32)]))
        remap = {int(t): i for i, t in enumerate(terms)}
        small = {}
        for f, (ptr, doc, w) in h.items():
            segs = [(doc[int(ptr[t]):int(ptr[t + 1])], w[int(ptr[t]):int(ptr[t + 1])]) for t in terms]
            sp = np.concatenate([[0], np.cumsum([len(s[0]) for s in segs])]).astype(np.uint64)
            small[f] = (sp, np.concatenate([s[0] for s in segs]), np.concatenate([s[1] for s in segs]))
        qt_small = np.array([remap[int(t)] for t in q_terms[:3 * ns]], np.uint32)
        sample_keys = sorted({(tuple(req[q]), tuple(exc[q])) for q in range(0, ns, 2)})
        allowed = np.stack([allowed_of(*key) for key in sample_keys])
        sid = np.array([sample_keys.index((tuple(req[q]), tuple(exc[q]))) if q % 2 == 0 else -1 for q in range(ns)], np.int32)
        ref, ref_n = masked_ref(oracle, ND, small["t"], small["b"], mt, mb, q_ptr[:ns + 1], qt_small, sid, allowed, k)
        assert_same_hits(hits[:ns], n_hits[:ns], ref, ref_n)
    finally:
        sc.close()
        ti.close()
        bi.close()
        del b_ptr, b_doc, b_tf, t_ptr, t_doc, t_tf
        torch.cuda.empty_cache()
