"""ss_diversify_hits beside ss_rerank_hits_by_vector on the same windows, measured like tools/vector_bench.py (library on a torch stream
shared with the caller, device buffers, blocks of back-to-back calls bracketed by synchronize, medians over blocks): 1024 queries, dim
128, page of 10, windows of 100 and 1000 rows of random docs.  Rows per window width: the re-rank; the diversified page with a query
vector; the same by rank (no query vector: no k_vec_hit_scores); and the diversified page of the whole window (k = k_in: every choice
is made), which shows what a choice costs.  Beside each diversify row two paper terms of k_div_gram: its products (tiles on and above
the diagonal, 2 * 64 * 64 * dim operations each) at 5e15 int8 operations per second, and the bytes of the Gram matrices it writes at
8 TB/s; and the groups the call ran in (option "div.scratch_bytes", default 256 MB).
    python tools/diversify_bench.py [--blocks 5] [--calls 5] [--docs 10000000] [--dim 128] [--queries 1024] [--k 10]"""
import argparse
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from spaghettisearch_amd import engine  # noqa: E402

HBM = 8e12          # bytes per second, the rate DESIGN.md's paper times use
I8_OPS = 5e15       # int8 matrix operations per second: twice the dense bf16 peak
SCRATCH = 256 << 20  # the default of "div.scratch_bytes" (csrc/diversify_plan.hpp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--docs", type=int, default=10_000_000)           # (smaller values: a rehearsal of the tool, not a measurement)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = engine.Context(0)
    stream = torch.cuda.Stream(device=dev)
    ctx.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        nd, dim, nq, k = a.docs, a.dim, a.queries, a.k
        tiny = (np.array([0, 1], np.uint64), np.array([0], np.uint32), np.array([1.0], np.float32))      # the lexical tables do not matter
        ti, bi = engine.InvertedIndex(ctx, nd, *tiny), engine.InvertedIndex(ctx, nd, *tiny)
        ti.set_weighted(np.ones(nd))
        bi.set_weighted(np.ones(nd))
        sc = engine.Scorer(ctx, ti, bi)
        gen = torch.Generator(device=dev).manual_seed(7)
        vec = torch.randint(-128, 128, (nd, dim), dtype=torch.int8, device=dev, generator=gen)
        sc.set_doc_vectors(vec)
        del vec
        rng = np.random.default_rng(8)
        qvec = torch.randint(-128, 128, (nq, dim), dtype=torch.int8, device=dev, generator=gen)

        def measure(name, call, extra):
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
            med = float(np.median(blocks))
            print(json.dumps({"row": name, "ms_median": round(med, 4), "ms_blocks": [round(x, 4) for x in blocks], **extra(med)}), flush=True)
            return med

        for k_in in (100, 1000):
            hits = np.zeros((nq, k_in), engine.HIT_DTYPE)
            hits["doc"] = rng.integers(0, nd, (nq, k_in))
            d_hits = torch.from_numpy(hits.view(np.uint8)).to(dev)
            d_n = torch.full((nq,), k_in, dtype=torch.int32, device=dev)

            def page(kk):
                return (torch.empty(nq * kk * 40, dtype=torch.uint8, device=dev), torch.empty(nq, dtype=torch.int32, device=dev),
                        torch.empty(nq * kk * 2, dtype=torch.int32, device=dev))
            p_rr = (torch.empty(nq * k * 40, dtype=torch.uint8, device=dev), torch.empty(nq, dtype=torch.int32, device=dev),
                    torch.empty(nq * k, dtype=torch.int32, device=dev))
            p_k, p_all = page(k), page(k_in)
            tiles = -(-k_in // 64)
            pitch = tiles * 64
            prod_ms = nq * (tiles * (tiles + 1) // 2) * 2 * 64 * 64 * dim / I8_OPS * 1e3
            write_ms = nq * k_in * k_in * 4 / HBM * 1e3
            group = max(1, min(SCRATCH // (pitch * pitch * 4), nq, 65535))
            paper = {"gram_products_at_5e15_ms": round(prod_ms, 4), "gram_bytes_written_at_8TBs_ms": round(write_ms, 4), "groups": -(-nq // group)}
            rr = measure(f"ss_rerank_hits_by_vector n_q={nq} k_in={k_in} k={k}",
                         lambda: sc.rerank_hits_by_vector(qvec, d_hits, d_n, k, k_in=k_in, out=p_rr), lambda med: {})
            over = lambda med: {**paper, "over_rerank": round(med / rr, 1)}       # noqa: E731
            measure(f"ss_diversify_hits n_q={nq} k_in={k_in} k={k} qvec w=2:1",
                    lambda: sc.diversify_hits(qvec, d_hits, d_n, k, 2, 1, k_in=k_in, out=p_k), over)
            measure(f"ss_diversify_hits n_q={nq} k_in={k_in} k={k} by rank w=30:1",
                    lambda: sc.diversify_hits(None, d_hits, d_n, k, 30, 1, k_in=k_in, out=p_k), over)
            measure(f"ss_diversify_hits n_q={nq} k_in={k_in} k={k_in} qvec w=2:1 (every choice)",
                    lambda: sc.diversify_hits(qvec, d_hits, d_n, k_in, 2, 1, k_in=k_in, out=p_all), over)
        sc.close()
        ti.close()
        bi.close()
    ctx.set_stream(None)
    ctx.close()


if __name__ == "__main__":
    main()
