"""Query operators at BASELINE config 3 (10M docs, 1024 x 3-term OR queries, k = 100): ms per batch with results in HBM, measured
like tools/mask_bench.py (library on a torch stream shared with the caller, blocks of back-to-back calls bracketed by synchronize).
Rows: the unconstrained batch (ss_score_topk, and ss_score_topk_constrained with empty constraint arrays), then every query of the
batch with one excluded head term, one excluded tail term, one required tail term outside the query, one of its own terms required,
and 1024 distinct excluded tail terms (one set per query) against one shared one.  Every row also prints the bytes k_constraint_masks
moves (one read of each set's constraint lists + one write of its words) and what that takes at 8 TB/s.
    python tools/constraint_bench.py [--blocks 6] [--calls 20] [--rows 0,2,5]"""
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
    ap.add_argument("--rows", default="", help="comma-separated row numbers (default: all)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = engine.Context(0)
    stream = torch.cuda.Stream(device=dev)
    ctx.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        nd, nt = 10_000_000, 1_000_000
        b = synth.zipf_index_torch(nd, nt, 640_000_000, seed=44, device=dev)
        t = synth.zipf_index_torch(nd, nt, 40_000_000, seed=144, device=dev)
        df = (b[0][1:] - b[0][:-1] + t[0][1:] - t[0][:-1]).cpu().numpy().astype(np.int64)     # title + body postings per term
        bi = engine.InvertedIndex(ctx, nd, *b)
        ti = engine.InvertedIndex(ctx, nd, *t)
        del b, t
        ti.tfidf_build(nd, False, False, False)
        bi.tfidf_build(nd, False, False, False)
        sc = engine.Scorer(ctx, ti, bi)
        k, nq = 100, 1024
        q_ptr, q_terms = synth.make_queries(nq, 3, 10000, seed=45)
        d_hits = torch.empty(nq * k * 40, dtype=torch.uint8, device=dev)
        d_n = torch.empty(nq, dtype=torch.int32, device=dev)
        n_words = (nd + 31) // 32
        none = [[] for _ in range(nq)]
        head, tail = 0, 5000
        rows = [("unconstrained score_topk", None, None),
                ("unconstrained, empty constraint arrays", none, none),
                ("one excluded head term (shared)", None, [[head]] * nq),
                ("one excluded tail term (shared)", None, [[tail]] * nq),
                ("one required tail term outside the query (shared)", [[tail]] * nq, None),
                ("a required query term (its first)", [[int(q_terms[q_ptr[q]])] for q in range(nq)], None),
                ("1024 distinct sets: excluded tail term 1000 + q", None, [[1000 + q] for q in range(nq)]),
                ("1 shared set: excluded tail term 1000", None, [[1000]] * nq)]
        pick = [int(x) for x in a.rows.split(",")] if a.rows else range(len(rows))

        def pack(lists):
            if lists is None:
                return None
            return (np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint32),
                    np.array([t for x in lists for t in x], np.uint32))

        for i in pick:
            name, req, exc = rows[i]
            r, e = pack(req), pack(exc)

            def call():
                if req is None and exc is None:
                    sc.score_topk(q_ptr, q_terms, k, out=(d_hits, d_n))
                else:
                    sc.score_topk_constrained(q_ptr, q_terms, k, req=r, exc=e, out=(d_hits, d_n))

            sets = {(tuple(sorted(set(req[q]))) if req else (), tuple(sorted(set(exc[q]))) if exc else ()) for q in range(nq)}
            sets.discard(((), ()))
            build_bytes = sum(4 * sum(int(df[x]) for x in rr + ee) + 4 * n_words for rr, ee in sets)
            for _ in range(3):
                call()
            blocks = []
            for _ in range(a.blocks):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    call()
                torch.cuda.synchronize()
                blocks.append((time.perf_counter() - t0) / a.calls * 1e3)
            n_hits = d_n.cpu().numpy()
            print(json.dumps({"row": i, "batch": name, "sets": len(sets), "ms_per_batch_median": round(float(np.median(blocks)), 4),
                              "ms_per_batch_blocks": [round(x, 4) for x in blocks],
                              "build_bytes": build_bytes, "build_us_at_8TBps": round(build_bytes / 8e12 * 1e6, 2),
                              "mean_hits_per_query": round(float(n_hits.mean()), 2)}), flush=True)
        sc.close()
        ti.close()
        bi.close()
    ctx.set_stream(None)
    ctx.close()


if __name__ == "__main__":
    main()
