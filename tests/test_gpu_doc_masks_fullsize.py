"""Doc allow-lists at BASELINE config 3's full size (10M docs / 1M terms / 641M+41M postings, inputs generated on the device):
ss_score_topk_masked against the posting-deleted oracle (tests/test_gpu_doc_masks.py) on a sample of the batch."""
import numpy as np
import pytest

from spaghettisearch_amd import engine, synth
from tests.test_gpu_doc_masks import masked_ref
from tests.test_gpu_score import assert_same_hits

pytestmark = pytest.mark.gpu


def test_full_size_config3(ss_ctx, oracle):
    """BASELINE config 3 (10M docs, 1024 x 3-term OR, k = 100) with a 10 % allow-list on every other query, against the
    posting-deleted oracle on a sample of the batch (the sample's lists only: the oracle sees a table of those terms)."""
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
        allowed = np.random.default_rng(9).random(ND) < 0.1
        sc.set_doc_masks(engine.pack_doc_masks(allowed[None, :], ND))
        q_ptr, q_terms = synth.make_queries(1024, 3, 10_000, seed=45)
        mask_id = np.where(np.arange(1024) % 2 == 0, 0, -1).astype(np.int32)
        hits, n_hits = sc.score_topk_masked(q_ptr, q_terms, mask_id, 100)
        plain, pn = sc.score_topk(q_ptr, q_terms, 100)
        assert hits[1::2].tobytes() == plain[1::2].tobytes() and n_hits[1::2].tolist() == pn[1::2].tolist()
        ns = 24
        terms = np.unique(q_terms[:3 * ns])
        remap = {int(t): i for i, t in enumerate(terms)}
        h = {"b": (b_ptr.cpu().numpy().view(np.uint64), b_doc.cpu().numpy().view(np.uint32), wb),
             "t": (t_ptr.cpu().numpy().view(np.uint64), t_doc.cpu().numpy().view(np.uint32), wt)}
        small = {}
        for f, (ptr, doc, w) in h.items():
            segs = [(doc[int(ptr[t]):int(ptr[t + 1])], w[int(ptr[t]):int(ptr[t + 1])]) for t in terms]
            sp = np.concatenate([[0], np.cumsum([len(s[0]) for s in segs])]).astype(np.uint64)
            small[f] = (sp, np.concatenate([s[0] for s in segs]), np.concatenate([s[1] for s in segs]))
        qt_small = np.array([remap[int(t)] for t in q_terms[:3 * ns]], np.uint32)
        ref, ref_n = masked_ref(oracle, ND, small["t"], small["b"], mt, mb, q_ptr[:ns + 1], qt_small, mask_id[:ns],
                                allowed[None, :], 100)
        assert_same_hits(hits[:ns], n_hits[:ns], ref, ref_n)
        assert allowed[hits["doc"][0::2][:, :50].astype(np.int64)].all()
    finally:
        sc.close()
        ti.close()
        bi.close()
        del b_ptr, b_doc, b_tf, t_ptr, t_doc, t_tf
        torch.cuda.empty_cache()
