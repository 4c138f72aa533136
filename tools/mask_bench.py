"""Doc allow-lists at BASELINE config 3 (10M docs, 1024 x 3-term OR queries, k = 100): ms per batch with results in HBM, measured
like tools/score_wall.py (library on a torch stream shared with the caller, blocks of back-to-back calls bracketed by synchronize).
Rows: the unmasked batch (ss_score_topk, ss_score_topk_masked with every mask id -1, and ss_score_topk with the wave kernel off:
the k_score_slices route with its threshold floor), then the whole batch under one allow-list
of uniform density 100 / 50 / 10 / 1 %, and under a "category" list (one contiguous 3 % range of doc ids).
    python tools/mask_bench.py [--blocks 6] [--calls 20]"""
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
        sc = engine.Scorer(ctx, ti, bi)
        rng = np.random.default_rng(7)
        dens = [1.0, 0.5, 0.1, 0.01]
        allowed = np.zeros((len(dens) + 1, nd), dtype=bool)
        for i, d in enumerate(dens):
            allowed[i] = rng.random(nd) < d
        lo = int(nd * 0.40)
        allowed[len(dens), lo:lo + nd * 3 // 100] = True
        sc.set_doc_masks(engine.pack_doc_masks(allowed, nd))
        k, nq = 100, 1024
        q_ptr, q_terms = synth.make_queries(nq, 3, 10000, seed=45)
        d_hits = torch.empty(nq * k * 40, dtype=torch.uint8, device=dev)
        d_n = torch.empty(nq, dtype=torch.int32, device=dev)
        rows = [("unmasked score_topk", None), ("unmasked, mask ids -1", -1), ("unmasked, score.wave = 0 (slices route with floor)", "slices")] + \
               [(f"uniform {int(d * 100)} %", i) for i, d in enumerate(dens)] + [("category 3 % (contiguous ids)", len(dens))]

        def call(m):
            if m in (None, "slices"):
                sc.score_topk(q_ptr, q_terms, k, out=(d_hits, d_n))
            else:
                sc.score_topk_masked(q_ptr, q_terms, np.full(nq, m, np.int32), k, out=(d_hits, d_n))

        for name, m in rows:
            ctx.set_option("score.wave", 0 if m == "slices" else None)
            for _ in range(3):
                call(m)
            blocks = []
            for _ in range(a.blocks):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    call(m)
                torch.cuda.synchronize()
                blocks.append((time.perf_counter() - t0) / a.calls * 1e3)
            n_hits = d_n.cpu().numpy()
            print(json.dumps({"mask": name, "density": float(allowed[m].mean()) if isinstance(m, int) and m >= 0 else 1.0,
                              "ms_per_batch_median": round(float(np.median(blocks)), 4),
                              "ms_per_batch_blocks": [round(x, 4) for x in blocks],
                              "mean_hits_per_query": round(float(n_hits.mean()), 2)}), flush=True)
        sc.close()
        ti.close()
        bi.close()
    ctx.set_stream(None)
    ctx.close()


if __name__ == "__main__":
    main()
