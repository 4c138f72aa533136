"""ss_maxsim_topk, measured like tools/maxsim_bench.py (library on a torch stream shared with the caller, device buffers, blocks of
back-to-back calls bracketed by synchronize, medians over blocks): the benchmark's 10M docs of which --token-docs (default 1M) have 50 ..
150 token vectors of dim 128 (12.8 GB), 1024 queries of 32 token vectors, k = 10 and 100.  Beside each row three floors: the table's
bytes once per block of queries over 6.0 TB/s (MI355X_MICROARCH.md: a table swept in order from HBM), the 16x16x64 products the kernel
issues at 5e15 int8 operations per second, and the B tiles it reads from LDS (one ds_read_b128 of a wave per product) at 150 TB/s.
Then the same call under allow-lists of 1 % and 10 % of the docs; the only route without the call — ss_hit_maxsim_scores over every
doc in windows of 1024 rows (built on the device) with the scores copied back and the selection on the host — on a table cut to
--emulate-docs docs with tokens, with the call's time on that table beside it; and a passage-level table of 3 .. 10 tokens per doc.
    python tools/maxsim_topk_bench.py [--blocks 3] [--calls 1] [--docs 10000000] [--token-docs 1000000] [--emulate-docs 100000]
                                      [--passage-docs 10000000] [--dim 128] [--queries 1024] [--query-tokens 32]"""
import argparse
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from spaghettisearch_amd import engine  # noqa: E402

STREAM = 6.0e12     # bytes per second: a table far larger than the Infinity Cache swept in order
I8_OPS = 5e15       # int8 matrix operations per second: twice the dense bf16 peak
LDS_READ = 150e12   # bytes per second: ds_read_b128 with every CU streaming
WINDOW = 1024       # SS_MAX_TOPK: the rows of one ss_hit_maxsim_scores window


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--calls", type=int, default=1)
    ap.add_argument("--docs", type=int, default=10_000_000)           # (smaller values: a rehearsal of the tool, not a measurement)
    ap.add_argument("--token-docs", type=int, default=1_000_000)
    ap.add_argument("--emulate-docs", type=int, default=100_000)
    ap.add_argument("--passage-docs", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--query-tokens", type=int, default=32)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = engine.Context(0)
    stream = torch.cuda.Stream(device=dev)
    ctx.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        nd, dim, nq, m_q = a.docs, a.dim, a.queries, a.query_tokens
        tiny = (np.array([0, 1], np.uint64), np.array([0], np.uint32), np.array([1.0], np.float32))      # the lexical tables do not matter
        ti, bi = engine.InvertedIndex(ctx, nd, *tiny), engine.InvertedIndex(ctx, nd, *tiny)
        ti.set_weighted(np.ones(nd))
        bi.set_weighted(np.ones(nd))
        sc = engine.Scorer(ctx, ti, bi)
        gen = torch.Generator(device=dev).manual_seed(7)
        rng = np.random.default_rng(8)
        qtok = torch.randint(-128, 128, (nq * m_q, dim), dtype=torch.int8, device=dev, generator=gen)
        qt_ptr = (np.arange(nq + 1) * m_q).astype(np.uint32)
        qt = 1 if m_q <= 16 else 2 if m_q <= 32 else 4
        masks = np.zeros((2, nd), bool)
        masks[0] = rng.random(nd) < 0.01
        masks[1] = rng.random(nd) < 0.10
        sc.set_doc_masks(engine.pack_doc_masks(masks, nd))

        def set_table(counts, name):
            tok_ptr = np.zeros(nd + 1, np.uint64)
            tok_ptr[1:] = np.cumsum(counts)
            n_tok = int(tok_ptr[-1])
            tok = torch.randint(-128, 128, (n_tok, dim), dtype=torch.int8, device=dev, generator=gen)
            sc.set_doc_tokens(tok_ptr, tok)
            print(json.dumps({"table": name, "docs": nd, "docs_with_tokens": int((counts > 0).sum()), "tokens": n_tok, "table_bytes": n_tok * dim,
                              "dim": dim, "queries": nq, "query_tokens": m_q}), flush=True)

        def measure(name, call, extra):
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
            print(json.dumps({"row": name, "ms_median": round(med, 3), "ms_blocks": [round(x, 3) for x in blocks], **extra(med)}), flush=True)
            return med

        def floors(counts, allowed=None):
            """of one call: the bytes of the docs some query may take, once per block of 16 queries; the products of their 16-token tiles
            with every query's tiles of 16 slots; the B tiles those products read from LDS"""
            t = counts if allowed is None else counts[allowed]
            n_qblocks = -(-nq // 16)
            table = int(t.sum()) * dim
            products = int((-(-t // 16)).sum()) * (dim // 64) * qt * nq
            f = {"n_qblocks": n_qblocks, "bytes_read": table * n_qblocks, "byte_floor_at_6TBs_ms": round(table * n_qblocks / STREAM * 1e3, 3),
                 "products_at_5e15_ms": round(products * 2 * 16 * 16 * 64 / I8_OPS * 1e3, 3),
                 "lds_reads_at_150TBs_ms": round(products * 1024 / LDS_READ * 1e3, 3)}
            f["binding_floor"] = max(("byte_floor_at_6TBs_ms", "products_at_5e15_ms", "lds_reads_at_150TBs_ms"), key=lambda n: f[n])
            return f

        def outs(k):
            return torch.empty((nq, k, 2), dtype=torch.int32, device=dev), torch.empty(nq, dtype=torch.int32, device=dev)

        def over(f):
            return lambda med: {**f, "over_binding_floor": round(med / f[f["binding_floor"]], 2)}

        # ---- 1: the call itself, and 3a: allow-lists
        counts = np.zeros(nd, np.int64)
        n_tok_docs = min(a.token_docs, nd)
        counts[:n_tok_docs] = rng.integers(50, 151, n_tok_docs)
        set_table(counts, "50 .. 150 tokens per doc")
        for k in (10, 100):
            o = outs(k)
            measure(f"ss_maxsim_topk n_q={nq} m_q={m_q} k={k}", lambda: sc.maxsim_topk(qt_ptr, qtok, k, out=o), over(floors(counts)))
        o = outs(10)
        for mi, share in ((0, "1 %"), (1, "10 %")):
            mid = torch.full((nq,), mi, dtype=torch.int32, device=dev)
            measure(f"ss_maxsim_topk n_q={nq} m_q={m_q} k=10, allow-list of {share} of the docs",
                    lambda: sc.maxsim_topk(qt_ptr, qtok, 10, mask_id=mid, out=o), over(floors(counts, masks[mi])))

        # ---- 2: without the call: every doc through ss_hit_maxsim_scores in windows of 1024 rows, the selection on the host
        n_em = min(a.emulate_docs, n_tok_docs)
        counts[n_em:] = 0
        set_table(counts, f"cut to {n_em} docs with tokens")
        k = 10
        o = outs(k)
        new = measure(f"ss_maxsim_topk n_q={nq} m_q={m_q} k={k} ({n_em} docs with tokens)", lambda: sc.maxsim_topk(qt_ptr, qtok, k, out=o),
                      over(floors(counts)))
        want = o[0].cpu().numpy().copy()
        d_n = torch.full((nq,), WINDOW, dtype=torch.int32, device=dev)
        d_sc = torch.empty((nq, WINDOW), dtype=torch.int32, device=dev)
        d_hits = torch.zeros((nq, WINDOW, 10), dtype=torch.int32, device=dev)           # rows of 40 bytes, .doc first: built on the device
        d_rows = d_hits.view(torch.uint8).view(nq, WINDOW * 40)                           # (the same memory, as the engine takes rows)
        ramp = torch.arange(WINDOW, dtype=torch.int32, device=dev)
        rows = np.zeros((nq, k, 2), np.int32)

        def emulate():
            all_sc = np.empty((nq, n_em), np.int32)
            for d0 in range(0, n_em, WINDOW):
                n = min(WINDOW, n_em - d0)
                d_hits[:, :, 0] = torch.clamp(ramp + d0, max=n_em - 1)
                sc.hit_maxsim_scores(qt_ptr, qtok, d_rows, d_n, k_in=WINDOW, out=d_sc)
                all_sc[:, d0:d0 + n] = d_sc.cpu().numpy()[:, :n]
            key = (all_sc.astype(np.int64) << 32) + (0xFFFFFFFF - np.arange(n_em, dtype=np.int64))     # score descending, doc ascending
            top = np.sort(np.partition(key, n_em - k, axis=1)[:, n_em - k:], axis=1)[:, ::-1]
            rows[:, :, 0], rows[:, :, 1] = 0xFFFFFFFF - (top & 0xFFFFFFFF), top >> 32

        old = measure(f"ss_hit_maxsim_scores over every doc in windows of {WINDOW} rows + selection on the host, k={k} ({n_em} docs with tokens)",
                      emulate, lambda med: {"calls_per_batch": -(-n_em // WINDOW), "over_ss_maxsim_topk": round(med / new, 1)})
        assert rows.tobytes() == want.tobytes(), "the emulation and ss_maxsim_topk disagree"
        del old

        # ---- 3b: a passage-level table
        counts = np.zeros(nd, np.int64)
        n_pass = min(a.passage_docs, nd)
        counts[:n_pass] = rng.integers(3, 11, n_pass)
        set_table(counts, "3 .. 10 tokens per doc")
        o = outs(10)
        f = floors(counts)
        f["tile_rows_filled"] = round(float(counts.sum()) / float((-(-counts // 16) * 16).sum()), 3)
        measure(f"ss_maxsim_topk n_q={nq} m_q={m_q} k=10, passage-level table", lambda: sc.maxsim_topk(qt_ptr, qtok, 10, out=o), over(f))
        sc.close()
        ti.close()
        bi.close()
    ctx.set_stream(None)
    ctx.close()


if __name__ == "__main__":
    main()
