"""ss_hit_maxsim_scores and ss_rerank_hits_by_maxsim beside ss_rerank_hits_by_vector on the same windows, measured like
tools/diversify_bench.py (library on a torch stream shared with the caller, device buffers, blocks of back-to-back calls bracketed by
synchronize, medians over blocks): the benchmark's 10M docs, 1024 queries of 32 token vectors, dim 128, page of 10, windows of 100 and
1000 rows.  --token-docs of the docs (default 1M: 12.8 GB of tokens, far beyond every cache; all 10M would be 128 GB, twice while the
table is copied) have between 50 and 150 token vectors, and the windows draw their rows from those docs.  Beside each MaxSim row the
byte floor: the token bytes the call gathers over 5.5 TB/s, the rate MI355X_MICROARCH.md gives for random whole rows gathered once into
registers from a buffer far larger than the Infinity Cache; and the matrix-core term, its 16x16x64 products at 5e15 int8 operations
per second.  Then the sweep of option "maxsim.wide_tokens": 64 queries whose windows of 100 rows each hold one doc of 50,000 tokens.
    python tools/maxsim_bench.py [--blocks 5] [--calls 5] [--docs 10000000] [--token-docs 1000000] [--dim 128] [--queries 1024]
                                 [--query-tokens 32] [--k 10]"""
import argparse
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from spaghettisearch_amd import engine  # noqa: E402

GATHER = 5.5e12     # bytes per second: random whole rows, each fetched once, far beyond the Infinity Cache
I8_OPS = 5e15       # int8 matrix operations per second: twice the dense bf16 peak
WIDE_DOC_TOKENS = 50_000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--docs", type=int, default=10_000_000)           # (smaller values: a rehearsal of the tool, not a measurement)
    ap.add_argument("--token-docs", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--query-tokens", type=int, default=32)
    ap.add_argument("--k", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = engine.Context(0)
    stream = torch.cuda.Stream(device=dev)
    ctx.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        nd, dim, nq, k, m_q = a.docs, a.dim, a.queries, a.k, a.query_tokens
        n_tok_docs = min(a.token_docs, nd - 1)
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
        counts = np.zeros(nd, np.int64)
        counts[:n_tok_docs] = rng.integers(50, 151, n_tok_docs)
        counts[n_tok_docs] = WIDE_DOC_TOKENS                          # the one wide doc, behind the docs the windows draw from
        tok_ptr = np.zeros(nd + 1, np.uint64)
        tok_ptr[1:] = np.cumsum(counts)
        n_tok = int(tok_ptr[-1])
        tok = torch.randint(-128, 128, (n_tok, dim), dtype=torch.int8, device=dev, generator=gen)
        sc.set_doc_tokens(tok_ptr, tok)
        del tok
        print(json.dumps({"docs": nd, "docs_with_tokens": n_tok_docs + 1, "tokens": n_tok, "table_bytes": n_tok * dim + 8 * (nd + 1), "dim": dim,
                          "queries": nq, "query_tokens": m_q, "k": k}), flush=True)
        qvec = torch.randint(-128, 128, (nq, dim), dtype=torch.int8, device=dev, generator=gen)
        qtok = torch.randint(-128, 128, (nq * m_q, dim), dtype=torch.int8, device=dev, generator=gen)
        qt_ptr = (np.arange(nq + 1) * m_q).astype(np.uint32)

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

        def paper(docs):
            """the floor of one call over windows of these docs: bytes gathered, and 16x16x64 products (tiles of 16 tokens, padded to
            iterations of 64, times the query's tiles of 16 slots)"""
            t = counts[docs.reshape(-1)]
            qt = 1 if m_q <= 16 else 2 if m_q <= 32 else 4
            ops = int((-(-t // 64) * 4).sum()) * qt * (dim // 64) * 2 * 16 * 16 * 64
            gathered = int(t.sum()) * dim
            return {"token_bytes_gathered": gathered, "byte_floor_at_5.5TBs_ms": round(gathered / GATHER * 1e3, 4),
                    "products_at_5e15_ms": round(ops / I8_OPS * 1e3, 4)}

        def window(n_q, k_in, docs):
            hits = np.zeros((n_q, k_in), engine.HIT_DTYPE)
            hits["doc"] = docs
            return torch.from_numpy(hits.view(np.uint8)).to(dev), torch.full((n_q,), k_in, dtype=torch.int32, device=dev)

        def page(n_q, kk):
            return (torch.empty(n_q * kk * 40, dtype=torch.uint8, device=dev), torch.empty(n_q, dtype=torch.int32, device=dev),
                    torch.empty(n_q * kk, dtype=torch.int32, device=dev))

        for k_in in (100, 1000):
            docs = rng.integers(0, n_tok_docs, (nq, k_in))
            d_hits, d_n = window(nq, k_in, docs)
            p, o_sc = page(nq, k), torch.empty(nq * k_in, dtype=torch.int32, device=dev)
            floor = paper(docs)
            rr = measure(f"ss_rerank_hits_by_vector n_q={nq} k_in={k_in} k={k} (yardstick)",
                         lambda: sc.rerank_hits_by_vector(qvec, d_hits, d_n, k, k_in=k_in, out=p), lambda med: {})
            over = lambda med: {**floor, "over_byte_floor": round(med / (floor["token_bytes_gathered"] / GATHER * 1e3), 2),    # noqa: E731
                                "over_rerank_by_vector": round(med / rr, 1)}
            measure(f"ss_hit_maxsim_scores n_q={nq} m_q={m_q} k_in={k_in}",
                    lambda: sc.hit_maxsim_scores(qt_ptr, qtok, d_hits, d_n, k_in=k_in, out=o_sc), over)
            measure(f"ss_rerank_hits_by_maxsim n_q={nq} m_q={m_q} k_in={k_in} k={k}",
                    lambda: sc.rerank_hits_by_maxsim(qt_ptr, qtok, d_hits, d_n, k, k_in=k_in, out=p), over)
            ctx.set_option("maxsim.wide_tokens", 64)                  # what sharing costs rows that do not need it: most of these docs
            measure(f"ss_hit_maxsim_scores n_q={nq} m_q={m_q} k_in={k_in}, maxsim.wide_tokens=64 (most rows shared)",
                    lambda: sc.hit_maxsim_scores(qt_ptr, qtok, d_hits, d_n, k_in=k_in, out=o_sc), over)
            ctx.set_option("maxsim.wide_tokens", None)
        # ---- the option's sweep: one doc of 50,000 tokens in every window of 100 rows, 64 queries
        n_w, k_in = min(64, nq), 100
        docs = rng.integers(0, n_tok_docs, (n_w, k_in))
        docs[:, 17] = n_tok_docs
        d_hits, d_n = window(n_w, k_in, docs)
        o_sc = torch.empty(n_w * k_in, dtype=torch.int32, device=dev)
        floor = paper(docs)
        base = None
        for wide in (64, 256, 1024, 4096, 16384, 2 ** 30):
            ctx.set_option("maxsim.wide_tokens", wide)
            measure(f"ss_hit_maxsim_scores n_q={n_w} m_q={m_q} k_in={k_in}, one doc of {WIDE_DOC_TOKENS} tokens per window, maxsim.wide_tokens={wide}",
                    lambda: sc.hit_maxsim_scores(qt_ptr[:n_w + 1], qtok, d_hits, d_n, k_in=k_in, out=o_sc), lambda med: floor)
            got = o_sc.cpu().numpy().tobytes()
            base = base or got
            assert got == base, "the scores depend on maxsim.wide_tokens"
        ctx.set_option("maxsim.wide_tokens", None)
        sc.close()
        ti.close()
        bi.close()
    ctx.set_stream(None)
    ctx.close()


if __name__ == "__main__":
    main()
