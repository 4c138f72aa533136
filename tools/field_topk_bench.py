"""ss_field_topk beside its yardsticks, ss_facet_counts (totals only: the same match-set work, no selection) and ss_score_topk (k = 100),
on the benchmark's tables (bench.py's top-k half: 10M docs, 1M terms, 640M body and 40M title postings, seeds 44 / 144) and its three
batches of 1024 x 3-term queries (head, mixed, tail), measured like tools/facet_bench.py: library on a torch stream shared with the
caller, device buffers, blocks of back-to-back calls bracketed by synchronize, medians over blocks, after the settle wait bench.py
uses.  Rows per batch: pages of 10 and 100 and K = 1024; ascending on a random date column and descending on a column that rises
with the doc id (every later doc beats the threshold: the compaction's worst case); with and without one range clause.  Beside each
row: its ratio to the facet totals of the same batch and the paper time — the batch's posting doc ids once at 4 bytes each, the
distinct allowed sets once, 8 bytes per matched doc gathered, at 8 TB/s.  --yardsticks prints the yardstick rows alone (run from a
checkout of the parent commit, it gives the parent's times of the same batches).
    python tools/field_topk_bench.py [--blocks 5] [--calls 5] [--docs 10000000] [--settle 8] [--yardsticks] [--runs 0]"""
import argparse
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from spaghettisearch_amd import engine, synth  # noqa: E402

HBM = 8e12          # bytes per second, the rate DESIGN.md's paper times use


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--docs", type=int, default=10_000_000)           # (smaller values: a rehearsal of the tool, not a measurement)
    ap.add_argument("--terms", type=int, default=1_000_000)
    ap.add_argument("--body-postings", type=int, default=640_000_000)
    ap.add_argument("--title-postings", type=int, default=40_000_000)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--settle", type=float, default=8.0)              # seconds of idle in front of the first GPU call, as bench.py
    ap.add_argument("--yardsticks", action="store_true")
    ap.add_argument("--runs", type=int, default=0)                    # option "ftopk.runs" (0: the plan's choice)
    a = ap.parse_args()
    if a.settle > 0 and a.docs >= 10_000_000:
        time.sleep(a.settle)
    dev = torch.device("cuda", 0)
    ctx = engine.Context(0)
    stream = torch.cuda.Stream(device=dev)
    ctx.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        nd, nt, nq, k = a.docs, a.terms, a.queries, 100
        b = synth.zipf_index_torch(nd, nt, a.body_postings, seed=44, device=dev)
        t = synth.zipf_index_torch(nd, nt, a.title_postings, seed=144, device=dev)
        bi, ti = engine.InvertedIndex(ctx, nd, *b), engine.InvertedIndex(ctx, nd, *t)
        h_bptr, h_tptr = b[0].cpu().numpy().view(np.uint64), t[0].cpu().numpy().view(np.uint64)
        del b, t
        torch.cuda.empty_cache()
        ti.tfidf_build(nd, want_w=False, want_mag=False, want_idf=False)
        bi.tfidf_build(nd, want_w=False, want_mag=False, want_idf=False)
        sc = engine.Scorer(ctx, ti, bi)
        ctx.set_option("score.timing", 0)
        if not a.yardsticks and a.runs:
            ctx.set_option("ftopk.runs", a.runs)
        n_words = (nd + 31) // 32
        gen = torch.Generator(device=dev).manual_seed(9)
        # field 0: a random date column (days of age); field 1: rises with the doc id, as crawl order makes dates do
        cols = torch.stack([torch.randint(0, 3650, (nd,), dtype=torch.int64, device=dev, generator=gen),
                            torch.arange(nd, dtype=torch.int64, device=dev) * 7 + 1_000_000])
        sc.set_doc_fields(cols)
        del cols
        d_hits = torch.empty(nq * k * 40, dtype=torch.uint8, device=dev)
        d_nhits = torch.empty(nq, dtype=torch.int32, device=dev)
        d_match = torch.zeros(nq, dtype=torch.int32, device=dev)
        d_docs = torch.zeros(nq * 1024, dtype=torch.int32, device=dev)
        d_vals = torch.zeros(nq * 1024, dtype=torch.int64, device=dev)
        d_n = torch.zeros(nq, dtype=torch.int32, device=dev)

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

        for batch, top, seed in (("head", 10_000, 45), ("mixed", 100_000, 2045), ("tail", nt, 1045)):
            q_ptr, q_terms = synth.make_queries(nq, 3, min(top, nt), seed=seed)
            postings = int(sum((h_bptr[x + 1] - h_bptr[x]) + (h_tptr[x + 1] - h_tptr[x]) for x in q_terms.astype(np.int64)))
            measure(f"{batch}: ss_score_topk k={k}", lambda: sc.score_topk(q_ptr, q_terms, k, out=(d_hits, d_nhits)), lambda med: {"postings": postings})
            facet = measure(f"{batch}: ss_facet_counts totals only", lambda: sc.facet_counts(q_ptr, q_terms, out=(d_match, None, None)),
                            lambda med: {"paper_ms_at_8TBs": round(postings * 4 / HBM * 1e3, 4)})
            if a.yardsticks:
                continue
            one_clause = engine.pack_doc_ranges([[(0, 0, 3000)] for _ in range(nq)])     # one allowed set for the batch: ~82 % of the docs

            def row(name, field, desc, first, kk, ranges):
                out = (d_docs, d_n, d_vals, d_match)
                call = lambda: sc.field_topk(q_ptr, q_terms, field, desc, first, kk, ranges=ranges, out=out)      # noqa: E731
                call()
                torch.cuda.synchronize()
                matched = int(d_match.cpu().numpy().view(np.uint32).astype(np.int64).sum())

                def extra(med):
                    paper = (postings * 4 + (n_words * 4 if ranges is not None else 0) + matched * 8) / HBM * 1e3
                    return {"over_facet_totals": round(med / facet, 2), "matched_docs": matched, "paper_ms_at_8TBs": round(paper, 4),
                            "fraction_of_paper": round(paper / med, 3)}
                measure(f"{batch}: ss_field_topk {name}", call, extra)

            for first, kk in ((0, 10), (0, 100), (0, 1024)):
                row(f"random dates ascending, first {first} k {kk}", 0, False, first, kk, None)
                row(f"rising with doc id, descending, first {first} k {kk}", 1, True, first, kk, None)
            row("random dates ascending, first 0 k 10, one range clause", 0, False, 0, 10, one_clause)
            row("rising with doc id, descending, first 0 k 100, one range clause", 1, True, 0, 100, one_clause)
        sc.close()
        ti.close()
        bi.close()
    ctx.set_stream(None)
    ctx.close()


if __name__ == "__main__":
    main()
