"""ss_field_stats and ss_field_histogram beside their yardsticks, ss_facet_counts (totals only: the same match-set walk, no gather and no
counters) and ss_top_groups over 64 groups (the same walk with a 4-byte gather and an LDS histogram), on the benchmark's tables
(bench.py's top-k half: 10M docs, 1M terms, 640M body and 40M title postings, seeds 44 / 144) and its three batches of 1024 x 3-term
queries (head, mixed, tail), measured like tools/group_topk_bench.py: library on a torch stream shared with the caller, device buffers,
blocks of back-to-back calls bracketed by synchronize, medians over blocks, after the settle wait bench.py uses.  Rows per batch:
ss_field_stats for 1 and 4 fields; ss_field_histogram on a random date column and on a column rising with the doc id, at 240 bins by
explicit edges (calendar months), 4096 bins of a fixed width that is no power of two (the host's reciprocal, and `/` forced by
"fstats.plain_divide"), 4096 bins of a power-of-two width (a shift) and 65536 bins of a fixed width (global atomics; reciprocal and `/`).
Beside each row its ratio to the facet totals and to ss_top_groups at 64 groups of the same batch.
    python tools/field_stats_bench.py [--blocks 5] [--calls 5] [--docs 10000000] [--settle 8] [--runs 0]"""
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
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--docs", type=int, default=10_000_000)           # (smaller values: a rehearsal of the tool, not a measurement)
    ap.add_argument("--terms", type=int, default=1_000_000)
    ap.add_argument("--body-postings", type=int, default=640_000_000)
    ap.add_argument("--title-postings", type=int, default=40_000_000)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--settle", type=float, default=8.0)              # seconds of idle in front of the first GPU call, as bench.py
    ap.add_argument("--runs", type=int, default=0)                    # option "fstats.runs" (0: the plan's choice)
    a = ap.parse_args()
    if a.settle > 0 and a.docs >= 10_000_000:
        time.sleep(a.settle)
    dev = torch.device("cuda", 0)
    ctx = engine.Context(0)
    stream = torch.cuda.Stream(device=dev)
    ctx.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        nd, nt, nq, m = a.docs, a.terms, a.queries, 10
        b = synth.zipf_index_torch(nd, nt, a.body_postings, seed=44, device=dev)
        t = synth.zipf_index_torch(nd, nt, a.title_postings, seed=144, device=dev)
        bi, ti = engine.InvertedIndex(ctx, nd, *b), engine.InvertedIndex(ctx, nd, *t)
        del b, t
        torch.cuda.empty_cache()
        ti.tfidf_build(nd, want_w=False, want_mag=False, want_idf=False)
        bi.tfidf_build(nd, want_w=False, want_mag=False, want_idf=False)
        sc = engine.Scorer(ctx, ti, bi)
        ctx.set_option("score.timing", 0)
        if a.runs:
            ctx.set_option("fstats.runs", a.runs)
        rng = np.random.default_rng(12)
        months = np.arange("2000-01", "2020-02", dtype="datetime64[M]").astype("datetime64[s]").astype(np.int64)   # 241 edges: 240 months
        t0, t1 = int(months[0]), int(months[-1])
        F_DATE, F_RISING, F_SIZE, F_HOLES = 0, 1, 2, 3
        holes = rng.integers(t0, t1, nd)
        holes[rng.random(nd) < 0.1] = -(2 ** 63)                     # a tenth of the docs without a value
        sc.set_doc_fields(np.stack([rng.integers(t0, t1, nd), t0 + np.arange(nd, dtype=np.int64) * ((t1 - t0) // nd),
                                    np.exp(rng.normal(10.0, 1.5, nd)).astype(np.int64), holes]).astype(np.int64))
        sc.set_doc_groups(rng.integers(0, 64, nd).astype(np.uint32))
        sc.group_values()                                             # (builds the ranks: no measured call waits for them)
        d_match = torch.zeros(nq, dtype=torch.int32, device=dev)
        d_rows = torch.zeros(nq * m * 2, dtype=torch.int32, device=dev)
        d_n, d_ng, d_ug = (torch.zeros(nq, dtype=torch.int32, device=dev) for _ in range(3))
        d_stats = torch.zeros(nq * 4 * 5, dtype=torch.int64, device=dev)
        d_counts = torch.zeros(nq * 65536, dtype=torch.int32, device=dev)
        d_tails = torch.zeros(nq * 4, dtype=torch.int32, device=dev)

        def measure(name, call, extra):
            for _ in range(3):
                call()
            blocks = []
            for _ in range(a.blocks):
                torch.cuda.synchronize()
                s0 = time.perf_counter()
                for _ in range(a.calls):
                    call()
                torch.cuda.synchronize()
                blocks.append((time.perf_counter() - s0) / a.calls * 1e3)
            med = float(np.median(blocks))
            print(json.dumps({"row": name, "ms_median": round(med, 4), "ms_blocks": [round(x, 4) for x in blocks], **extra(med)}), flush=True)
            return med

        span = t1 - t0
        hists = [("240 bins by edges", dict(n_bins=240, edges=months), (0,)),
                 ("4096 bins, fixed width", dict(n_bins=4096, origin=t0, width=span // 4096 + 1), (0, 1)),
                 ("4096 bins, width 2^18", dict(n_bins=4096, origin=t0, width=2 ** 18), (0,)),
                 ("65536 bins, fixed width", dict(n_bins=65536, origin=t0, width=span // 65536 + 1), (0, 1))]
        for batch, top, seed in (("head", 10_000, 45), ("mixed", 100_000, 2045), ("tail", nt, 1045)):
            q_ptr, q_terms = synth.make_queries(nq, 3, min(top, nt), seed=seed)
            facet = measure(f"{batch}: ss_facet_counts totals only", lambda: sc.facet_counts(q_ptr, q_terms, out=(d_match, None, None)), lambda med: {})
            matched = int(d_match.cpu().numpy().view(np.uint32).astype(np.int64).sum())
            groups = measure(f"{batch}: ss_top_groups first 0 m {m}, 64 groups, LDS histogram",
                             lambda: sc.top_groups(q_ptr, q_terms, 0, m, out=(d_rows, d_n, d_ng, d_ug, d_match)), lambda med: {"matched_docs": matched})
            ratios = lambda med: {"over_facet_totals": round(med / facet, 2), "over_top_groups_64": round(med / groups, 2)}   # noqa: E731
            for fields in ([F_DATE], [F_DATE, F_RISING, F_SIZE, F_HOLES]):
                measure(f"{batch}: ss_field_stats {len(fields)} field(s)", lambda: sc.field_stats(q_ptr, q_terms, fields, out=(d_stats, d_match)), ratios)
            for col, field in (("random dates", F_DATE), ("rising with the doc id", F_RISING)):
                for name, kw, divides in hists:
                    for dv in divides:
                        ctx.set_option("fstats.plain_divide", dv)
                        form = "" if len(divides) == 1 else (", `/`" if dv else ", reciprocal")
                        measure(f"{batch}: ss_field_histogram {col}, {name}{form}",
                                lambda: sc.field_histogram(q_ptr, q_terms, field, out=(d_counts, d_tails), **kw), ratios)
                    ctx.set_option("fstats.plain_divide", None)
        sc.close()
        ti.close()
        bi.close()
    ctx.set_stream(None)
    ctx.close()


if __name__ == "__main__":
    main()
