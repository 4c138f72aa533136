"""Doc vectors at 10M docs, dim 128, k 100, measured like tools/doc_fields_bench.py (library on a torch stream shared with the caller,
device buffers, blocks of back-to-back calls bracketed by synchronize, medians over blocks).  Rows: (a) ss_vector_topk at n_q = 1, 64
and 1024, unmasked and under a 1 % allow-list; (b) ss_rerank_hits_by_vector behind 1024 queries at k_in = 100 and 1024.  Beside each
time of (a) two bounds: the byte bound, n_docs * dim * passes bytes at 8 TB/s (passes = blocks of queries, each reads the table once),
and the product bound, 2 * n_docs * dim * n_q operations at 5e15 per second (int8 = twice the dense bf16 rate of 2.5e15), and the ratio
of the time to the larger of the two.  Beside (b) the bytes of the gathered rows at 8 TB/s.
    python tools/vector_bench.py [--blocks 5] [--calls 5] [--docs 10000000] [--dim 128] [--k 100]"""
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


def query_block(n_q, k, dim):
    """queries of one k_vec_topk workgroup, as csrc/vector_plan.hpp picks it for a 160 KB LDS"""
    want = max(2 * k, k + 96)
    for budget in (80 << 10, 160 << 10):
        for qb in (64, 32, 16):
            if qb > 16 and n_q <= qb // 2:
                continue
            fixed = qb * (dim + 16) + qb * 8 + 4 * qb * 8 + qb * 4 + 1024 + 2048 + 64
            if budget > fixed and (budget - fixed) // (qb * 8) >= want:
                return qb
    return 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--docs", type=int, default=10_000_000)           # (smaller values: a rehearsal of the tool, not a measurement)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--k", type=int, default=100)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = engine.Context(0)
    stream = torch.cuda.Stream(device=dev)
    ctx.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        nd, dim, k = a.docs, a.dim, a.k
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
        mask = engine.pack_doc_masks((rng.random(nd) < 0.01)[None, :], nd)
        sc.set_doc_masks(mask)

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

        for nq in (1, 64, 1024):
            qvec = torch.randint(-128, 128, (nq, dim), dtype=torch.int8, device=dev, generator=gen)
            out = (torch.empty((nq, k, 2), dtype=torch.int32, device=dev), torch.empty(nq, dtype=torch.int32, device=dev))
            passes = -(-nq // query_block(nq, k, dim))
            byte_ms = nd * dim * passes / HBM * 1e3
            prod_ms = 2 * nd * dim * nq / I8_OPS * 1e3

            def bounds(med):
                return {"passes": passes, "byte_bound_ms": round(byte_ms, 4), "product_bound_ms": round(prod_ms, 4),
                        "ratio_to_larger_bound": round(med / max(byte_ms, prod_ms), 2)}
            measure(f"(a) ss_vector_topk n_q={nq} k={k} unmasked", lambda: sc.vector_topk(qvec, k, out=out), bounds)
            ids = np.zeros(nq, np.int32)                                          # (host ids: read on the host, uploaded through a pinned block)
            measure(f"(a) ss_vector_topk n_q={nq} k={k} 1% mask", lambda: sc.vector_topk(qvec, k, ids, out=out), bounds)
        nq, k_page = 1024, 50
        qvec = torch.randint(-128, 128, (nq, dim), dtype=torch.int8, device=dev, generator=gen)
        for k_in in (100, 1024):
            hits = np.zeros((nq, k_in), engine.HIT_DTYPE)
            hits["doc"] = rng.integers(0, nd, (nq, k_in))
            d_hits = torch.from_numpy(hits.view(np.uint8)).to(dev)
            d_n = torch.full((nq,), k_in, dtype=torch.int32, device=dev)
            page = (torch.empty(nq * k_page * 40, dtype=torch.uint8, device=dev), torch.empty(nq, dtype=torch.int32, device=dev),
                    torch.empty(nq * k_page, dtype=torch.int32, device=dev))
            gather_ms = nq * k_in * (dim + 40) / HBM * 1e3
            measure(f"(b) ss_rerank_hits_by_vector n_q={nq} k_in={k_in} k={k_page}",
                    lambda: sc.rerank_hits_by_vector(qvec, d_hits, d_n, k_page, k_in=k_in, out=page),
                    lambda med: {"gathered_bytes_at_8TBs_ms": round(gather_ms, 5), "ratio": round(med / gather_ms, 1)})
        sc.close()
        ti.close()
        bi.close()
    ctx.set_stream(None)
    ctx.close()


if __name__ == "__main__":
    main()
