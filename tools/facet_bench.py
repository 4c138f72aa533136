"""ss_facet_counts beside ss_score_topk (k = 100) on the benchmark's tables (bench.py's top-k half: 10M docs, 1M terms, 640M body and
40M title postings, seeds 44 / 144) and its three batches of 1024 x 3-term queries (head: terms of the 10k most frequent, mixed: of
100k, tail: of all), measured like the other tools: library on a torch stream shared with the caller, device buffers, blocks of
back-to-back calls bracketed by synchronize, medians over blocks, after the settle wait bench.py uses.  Rows per batch: the scoring
call; totals only (no masks, no buckets); facets (8 registered masks, 8 nested date buckets); constrained facets whose range clauses
give 1, 4 and 1024 distinct allowed sets.  Beside each facet row: its ratio to the scoring call of the same batch, and the paper time
— the batch's posting doc ids once at 4 bytes each, the distinct allowed sets and the masks once, 8 bytes per matched doc and field
gathered, at 8 TB/s — with the fraction of it reached.  --score-only prints the scoring rows alone (run from a checkout of the
parent commit, it gives the parent's time of the same batches).
    python tools/facet_bench.py [--blocks 5] [--calls 5] [--docs 10000000] [--settle 8] [--score-only]"""
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
    ap.add_argument("--score-only", action="store_true")
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
        n_words = (nd + 31) // 32
        gen = torch.Generator(device=dev).manual_seed(9)
        if not a.score_only:
            days = torch.randint(0, 3650, (1, nd), dtype=torch.int64, device=dev, generator=gen)      # a date column: days of age
            sc.set_doc_fields(days)
            del days
        buckets = [(0, 0, (1 << i) - 1) for i in range(1, 9)]             # nested: the past 1, 3, 7, .. 255 days
        d_hits = torch.empty(nq * k * 40, dtype=torch.uint8, device=dev)
        d_nhits = torch.empty(nq, dtype=torch.int32, device=dev)
        d_match = torch.zeros(nq, dtype=torch.int32, device=dev)
        d_mc = torch.zeros(nq * 8, dtype=torch.int32, device=dev)
        d_bc = torch.zeros(nq * 8, dtype=torch.int32, device=dev)

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
            score = measure(f"{batch}: ss_score_topk k={k}", lambda: sc.score_topk(q_ptr, q_terms, k, out=(d_hits, d_nhits)),
                            lambda med: {"postings": postings})
            if a.score_only:
                continue

            def facet_row(name, n_masks, n_buckets, clauses, n_sets):
                sc.set_doc_masks(torch.randint(-2 ** 31, 2 ** 31 - 1, (n_masks, n_words), dtype=torch.int32, device=dev, generator=gen)
                                 if n_masks else None)
                kw = dict(ranges=None if clauses is None else engine.pack_doc_ranges(clauses), buckets=buckets[:n_buckets] if n_buckets else None,
                          out=(d_match, d_mc if n_masks else None, d_bc if n_buckets else None))
                call = lambda: sc.facet_counts(q_ptr, q_terms, **kw)      # noqa: E731
                call()
                torch.cuda.synchronize()
                matched = int(d_match.cpu().numpy().view(np.uint32).astype(np.int64).sum())

                def extra(med):
                    paper_bytes = postings * 4 + (n_sets + n_masks) * n_words * 4 + (matched * 8 if n_buckets else 0)
                    paper = paper_bytes / HBM * 1e3
                    return {"over_score_topk": round(med / score, 2), "matched_docs": matched, "paper_ms_at_8TBs": round(paper, 4),
                            "fraction_of_paper": round(paper / med, 3)}
                measure(f"{batch}: ss_facet_counts {name}", call, extra)

            facet_row("totals only", 0, 0, None, 0)
            facet_row("8 masks + 8 nested date buckets", 8, 8, None, 0)
            for n_sets in (1, 4, 1024):
                clauses = [[(0, 0, 3649 - (q % n_sets))] for q in range(nq)]
                facet_row(f"8 masks + 8 buckets, {n_sets} distinct allowed set(s)", 8, 8, clauses, n_sets)
            sc.set_doc_masks(None)
        sc.close()
        ti.close()
        bi.close()
    ctx.set_stream(None)
    ctx.close()


if __name__ == "__main__":
    main()
