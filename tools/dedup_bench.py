"""Near-duplicate results at BASELINE config 3 (10M docs, 640M body postings, 1024 x 3-term OR queries), measured like
tools/collapse_bench.py (library on a torch stream shared with the caller, blocks of back-to-back calls bracketed by synchronize).
Rows: (a) ss_index_build_doc_view and ss_index_build_signatures at n_slots = 8, 16, 32 on the body table, ms per build, beside the
paper figures of the signature pass (4 B per posting at 8 TB/s; n_slots x 9 integer ops per posting — an add, the mix's seven and
a minimum — over 256 CUs x 64 lanes x 2.4 GHz); (b) ss_score_topk at k = k_in in {100, 1024} with device buffers, then on those
rows ss_dedup_hits (min_match = n_slots / 2, k = 50) and ss_collapse_hits (g = 2, k = 50), the existing kernel of the same shape.
    python tools/dedup_bench.py [--blocks 6] [--calls 20] [--docs 10000000]"""
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
    ap.add_argument("--docs", type=int, default=10_000_000)           # (smaller values: a rehearsal of the tool, not a measurement)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = engine.Context(0)
    stream = torch.cuda.Stream(device=dev)
    ctx.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        nd = a.docs
        nt = nd // 10
        b = synth.zipf_index_torch(nd, nt, nd * 64, seed=44, device=dev)
        t = synth.zipf_index_torch(nd, nt, nd * 4, seed=144, device=dev)
        bi = engine.InvertedIndex(ctx, nd, *b)
        ti = engine.InvertedIndex(ctx, nd, *t)
        del b, t
        ti.tfidf_build(nd, False, False, False)
        bi.tfidf_build(nd, False, False, False)
        P = bi.n_post

        def timed(call, n):
            out = []
            for _ in range(n):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                torch.cuda.synchronize()
                out.append((time.perf_counter() - t0) * 1e3)
            return out
        # ---- (a) the builds
        views = timed(bi.build_doc_view, a.builds)
        print(json.dumps({"row": "(a) ss_index_build_doc_view(body)", "postings": P, "ms": [round(x, 2) for x in views]}), flush=True)
        dp = np.zeros(nd + 1, dtype=np.uint64)
        engine.check(ctx.lib.ss_index_read_doc_view(bi.h, dp.ctypes.data, None, None), ctx.h)
        lens = np.diff(dp.astype(np.int64))
        print(json.dumps({"row": "view row lengths", "mean": round(float(lens.mean()), 1), "p50": int(np.median(lens)), "p99": int(np.percentile(lens, 99)),
                          "max": int(lens.max()), "rows_over_32": int((lens > 32).sum()), "rows_over_1024": int((lens > 1024).sum())}), flush=True)
        for n_slots in (8, 16, 32):
            ms = timed(lambda: bi.build_signatures(n_slots), a.builds)
            best = min(ms)
            print(json.dumps({"row": f"(a) ss_index_build_signatures(body, {n_slots})", "ms": [round(x, 2) for x in ms],
                              "paper_memory_ms": round(P * 4 / 8e12 * 1e3, 3),
                              "paper_valu_ms": round(P * n_slots * 9 / (256 * 64 * 2.4e9) * 1e3, 3),
                              "postings_per_s": round(P / (best * 1e-3), 0), "int_ops_per_s": round(P * n_slots * 9 / (best * 1e-3), 0)}), flush=True)
        n_slots = 16
        bi.build_signatures(n_slots)
        # ---- (b) the walk behind a scoring batch
        sc = engine.Scorer(ctx, ti, bi)
        rng = np.random.default_rng(7)
        n_sites = max(1, nd // 50)
        sc.set_doc_groups((n_sites * rng.random(nd) ** 3).astype(np.uint32))
        nq, k_page = 1024, 50
        q_ptr, q_terms = synth.make_queries(nq, 3, nt // 100, seed=45)
        d_hits = torch.empty(nq * 1024 * 40, dtype=torch.uint8, device=dev)
        d_n = torch.empty(nq, dtype=torch.int32, device=dev)
        page_out = (torch.empty(nq * k_page * 40, dtype=torch.uint8, device=dev), torch.empty(nq, dtype=torch.int32, device=dev),
                    torch.empty(nq * k_page, dtype=torch.int32, device=dev), torch.empty(nq, dtype=torch.int32, device=dev))

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
            print(json.dumps({"row": name, "ms_per_batch_median": round(float(np.median(blocks)), 4),
                              "ms_per_batch_blocks": [round(x, 4) for x in blocks], **extra()}), flush=True)

        def page_extra():
            return {"mean_page_rows": round(float(page_out[1].cpu().numpy().mean()), 2), "mean_kept": round(float(page_out[3].cpu().numpy().mean()), 2)}
        for kw in (100, 1024):
            measure(f"(b) score_topk k={kw}", lambda: sc.score_topk(q_ptr, q_terms, kw, out=(d_hits, d_n)),
                    lambda: {"mean_hits_per_query": round(float(d_n.cpu().numpy().mean()), 2)})
            # (the rows of the scoring call are still in d_hits / d_n)
            for mm in (n_slots // 2, n_slots):
                measure(f"(b) dedup_hits k_in={kw} n_slots={n_slots} min_match={mm} k={k_page}",
                        lambda: sc.dedup_hits(d_hits, d_n, mm, k_page, k_in=kw, out=page_out), page_extra)
            measure(f"(b) collapse_hits k_in={kw} g=2 k={k_page}", lambda: sc.collapse_hits(d_hits, d_n, 2, k_page, k_in=kw, out=page_out), page_extra)
        sc.close()
        ti.close()
        bi.close()
    ctx.set_stream(None)
    ctx.close()


if __name__ == "__main__":
    main()
