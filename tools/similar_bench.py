"""Similar pages at BASELINE config 3 (10M docs, body table of 640M postings, k = 100), measured like tools/mask_bench.py (library on
a torch stream shared with the caller, blocks of back-to-back calls bracketed by synchronize):
  - ss_index_build_doc_view of the body table: ms per build, against the algorithmic bytes (read post_doc and post_w, write doc_term
    and doc_w: 16 bytes per posting) at 8 TB/s;
  - a 1024-seed batch of ss_similar_topk at m = 5, k = 100 with device outputs, and the SAME 1024 queries through ss_score_topk at
    k = 101: the overhead of the new call is the difference of the two;
  - --kernels-only: a short run of the new call alone, for `rocprofv3 --kernel-trace --stats -- python tools/similar_bench.py
    --kernels-only` (k_doc_top_terms and k_drop_seed in the kernel statistics).
    python tools/similar_bench.py [--blocks 6] [--calls 20] [--builds 3]"""
import argparse
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from spaghettisearch_amd import engine, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--builds", type=int, default=3)
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
        P = bi.n_post
        builds = []
        for _ in range(1 if a.kernels_only else a.builds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            bi.build_doc_view()
            torch.cuda.synchronize()
            builds.append((time.perf_counter() - t0) * 1e3)
        algo = 16 * P
        print(json.dumps({"what": "ss_index_build_doc_view(body)", "postings": P, "ms": [round(x, 2) for x in builds],
                          "algorithmic_bytes": algo, "ms_at_8TBps": round(algo / 8e12 * 1e3, 2),
                          "resident_bytes": 8 * P + 8 * (nd + 1)}), flush=True)
        sc = engine.Scorer(ctx, ti, bi)
        k, nq, m = 100, 1024, 5
        rng = np.random.default_rng(7)
        seeds = rng.integers(0, nd, size=nq).astype(np.uint32)
        terms, _, cnt = bi.doc_top_terms(seeds, m, want_w=False)
        q_ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
        q_terms = np.concatenate([terms[i, :cnt[i]] for i in range(nq)]).astype(np.uint32)
        d_hits = torch.empty(nq * (k + 1) * 40, dtype=torch.uint8, device=dev)
        d_n = torch.empty(nq, dtype=torch.int32, device=dev)
        rows = [("ss_similar_topk m=5 k=100", lambda: sc.similar_topk(seeds, k, m=m, out=(d_hits, d_n)))]
        if not a.kernels_only:
            rows.append(("ss_score_topk of the same queries, k=101", lambda: sc.score_topk(q_ptr, q_terms, k + 1, out=(d_hits, d_n))))
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
                              "ms_per_batch_blocks": [round(x, 4) for x in blocks], "mean_terms_per_seed": round(float(cnt.mean()), 2),
                              "mean_hits_per_query": round(float(d_n.cpu().numpy().mean()), 2)}), flush=True)
        sc.close()
        ti.close()
        bi.close()
    ctx.set_stream(None)
    ctx.close()


if __name__ == "__main__":
    main()
