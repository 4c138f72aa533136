"""Related terms at BASELINE config 3 (10M docs, body table of 640M postings; the benchmark's 1024 three-term queries), measured
like tools/similar_bench.py (library on a torch stream shared with the caller, blocks of back-to-back calls bracketed by synchronize):
  - a 1024-query batch of ss_related_terms at (k_fb, m_doc, m) = (10, 5, 10) with device outputs;
  - the SAME answer composed from the existing public calls on the same build: ss_score_topk at k = 10 with host outputs ->
    ss_index_doc_top_terms of the 10240 hits with host outputs -> a hash map per query on the host (Python dicts here: the
    aggregation time is reported apart from the two library calls, which are what a host in any language pays);
    the composed rows are checked against the call's, bit for bit;
  - ss_score_topk at k = 10 with device outputs alone: what the new call adds behind the scoring call is the difference;
  - --kernels-only: a short run of the new call alone, for `rocprofv3 --kernel-trace --stats -- python tools/related_bench.py
    --kernels-only` (k_hit_docs, k_doc_top_terms and k_related_terms in the kernel statistics).
    python tools/related_bench.py [--blocks 6] [--calls 20]"""
import argparse
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from spaghettisearch_amd import engine, synth  # noqa: E402


def aggregate(q_ptr, q_terms, rows, n_rows, t_hit, w_hit, cnt, m):
    """the host side of the composed answer: per query a map term -> float64 sum in rank order, then the m best"""
    n_q, k_fb = rows.shape
    m_doc = t_hit.shape[-1]
    t_hit, w_hit, cnt = t_hit.reshape(n_q, k_fb, m_doc), w_hit.reshape(n_q, k_fb, m_doc).astype(np.float64), cnt.reshape(n_q, k_fb)
    terms, score, n_out = np.zeros((n_q, m), np.uint32), np.zeros((n_q, m), np.float64), np.zeros(n_q, np.int32)
    for q in range(n_q):
        typed = set(q_terms[q_ptr[q]:q_ptr[q + 1]].tolist())
        sums = {}
        for j in range(int(n_rows[q])):
            for t, w in zip(t_hit[q, j, :cnt[q, j]].tolist(), w_hit[q, j, :cnt[q, j]].tolist()):
                if t not in typed:
                    sums[t] = sums.get(t, 0.0) + w
        best = sorted(sums.items(), key=lambda kv: (kv[1] != kv[1], -kv[1] if kv[1] == kv[1] else 0.0, kv[0]))[:m]
        n_out[q] = len(best)
        terms[q, :len(best)] = [t for t, _ in best]
        score[q, :len(best)] = [s for _, s in best]
    return terms, score, n_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = engine.Context(0)
    stream = torch.cuda.Stream(device=dev)
    ctx.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        nd, nt = 10_000_000, 1_000_000
        b = synth.zipf_index_torch(nd, nt, 640_000_000, seed=44, device=dev)
        t = synth.zipf_index_torch(nd, nt, 40_000_000, seed=144, device=dev)
        bi = engine.InvertedIndex(ctx, nd, *b)
        ti = engine.InvertedIndex(ctx, nd, *t)
        del b, t
        ti.tfidf_build(nd, False, False, False)
        bi.tfidf_build(nd, False, False, False)
        bi.build_doc_view()
        sc = engine.Scorer(ctx, ti, bi)
        nq, k_fb, m_doc, m = 1024, 10, 5, 10
        q_ptr, q_terms = synth.make_queries(nq, 3, min(10_000, nt), seed=45)
        d_terms = torch.zeros(nq * m, dtype=torch.int32, device=dev)
        d_score = torch.zeros(nq * m, dtype=torch.float64, device=dev)
        d_n = torch.zeros(nq, dtype=torch.int32, device=dev)
        d_hits = torch.empty(nq * k_fb * 40, dtype=torch.uint8, device=dev)
        d_nh = torch.empty(nq, dtype=torch.int32, device=dev)
        parts = {}

        def composed_calls():
            rows, n_rows = sc.score_topk(q_ptr, q_terms, k_fb)
            t_hit, w_hit, cnt = bi.doc_top_terms(np.ascontiguousarray(rows["doc"]).reshape(-1), m_doc)
            parts["x"] = (rows, n_rows, t_hit, w_hit, cnt)

        rows = [("ss_related_terms (10, 5, 10), device outputs",
                 lambda: sc.related_terms(q_ptr, q_terms, m=m, k_fb=k_fb, m_doc=m_doc, out=(d_terms, d_score, d_n)))]
        if not a.kernels_only:
            rows.append(("ss_score_topk k=10, device outputs", lambda: sc.score_topk(q_ptr, q_terms, k_fb, out=(d_hits, d_nh))))
            rows.append(("composed: ss_score_topk k=10 + ss_index_doc_top_terms, host outputs (library calls only)", composed_calls))
        for name, call in rows:
            for _ in range(3):
                call()
            blocks = []
            for _ in range(1 if a.kernels_only else a.blocks):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    call()
                torch.cuda.synchronize()
                blocks.append((time.perf_counter() - t0) / a.calls * 1e3)
            print(json.dumps({"call": name, "ms_per_batch_median": round(float(np.median(blocks)), 4),
                              "ms_per_batch_blocks": [round(x, 4) for x in blocks]}), flush=True)
        if not a.kernels_only:
            agg = []
            for _ in range(3):
                t0 = time.perf_counter()
                comp = aggregate(q_ptr, q_terms, *parts["x"], m)
                agg.append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize()
            got = (d_terms.cpu().numpy().view(np.uint32).reshape(nq, m), d_score.cpu().numpy().reshape(nq, m), d_n.cpu().numpy())
            same = all(x.tobytes() == y.tobytes() for x, y in zip(got, comp))
            print(json.dumps({"what": "host aggregation of the composed answer (Python dicts)", "ms": [round(x, 2) for x in agg],
                              "composed_equals_call_bit_for_bit": same, "mean_terms_per_query": round(float(got[2].mean()), 2)}), flush=True)
        sc.close()
        ti.close()
        bi.close()
    ctx.set_stream(None)
    ctx.close()


if __name__ == "__main__":
    main()
