"""ss_top_groups beside its yardsticks, ss_facet_counts (totals only: the same match-set walk, no gather and no counters) and
ss_score_topk (k = 100), on the benchmark's tables (bench.py's top-k half: 10M docs, 1M terms, 640M body and 40M title postings, seeds
44 / 144) and its three batches of 1024 x 3-term queries (head, mixed, tail), measured like tools/field_topk_bench.py: library on a
torch stream shared with the caller, device buffers, blocks of back-to-back calls bracketed by synchronize, medians over blocks, after
the settle wait bench.py uses.  Rows per batch, at first 0, m 10: a table of 64 groups (the LDS histogram by default), 100k groups
assigned in clustered runs of 1 .. 200 docs, and 100k groups assigned at random (global atomics by default; the worst case for the
run-length merge); each also with the other path forced where the table admits it ("gtopk.lds_groups" 0 for the 64 groups; the 100k
tables do not fit the histogram).  Beside each row: its ratio to the facet totals of the same batch and the paper time — the batch's
posting doc ids once at 4 bytes each, 4 bytes of rank per matched doc, the counter rows zeroed once and read once, at 8 TB/s.
--yardsticks prints the yardstick rows alone (run from a checkout of the parent commit, it gives the parent's times of the same
batches).
    python tools/group_topk_bench.py [--blocks 5] [--calls 5] [--docs 10000000] [--settle 8] [--yardsticks] [--runs 0]"""
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
    ap.add_argument("--groups", type=int, default=100_000)
    ap.add_argument("--settle", type=float, default=8.0)              # seconds of idle in front of the first GPU call, as bench.py
    ap.add_argument("--yardsticks", action="store_true")
    ap.add_argument("--runs", type=int, default=0)                    # option "gtopk.runs" (0: the plan's choice)
    a = ap.parse_args()
    if a.settle > 0 and a.docs >= 10_000_000:
        time.sleep(a.settle)
    dev = torch.device("cuda", 0)
    ctx = engine.Context(0)
    stream = torch.cuda.Stream(device=dev)
    ctx.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        nd, nt, nq, k, m = a.docs, a.terms, a.queries, 100, 10
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
            ctx.set_option("gtopk.runs", a.runs)
        d_hits = torch.empty(nq * k * 40, dtype=torch.uint8, device=dev)
        d_nhits = torch.empty(nq, dtype=torch.int32, device=dev)
        d_match = torch.zeros(nq, dtype=torch.int32, device=dev)

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

        tables = []
        if not a.yardsticks:
            rng = np.random.default_rng(12)
            lens = rng.integers(1, 201, nd // 50)                       # clustered runs of 1 .. 200 docs, as crawl order clusters a site's docs
            lens = lens[:int(np.searchsorted(np.cumsum(lens), nd)) + 1]
            site = rng.integers(0, a.groups, len(lens)).astype(np.uint32)
            tables = [("64 groups at random", rng.integers(0, 64, nd).astype(np.uint32), (None, 0)),
                      (f"{a.groups} groups in clustered runs", np.repeat(site, lens)[:nd].copy(), (None,)),
                      (f"{a.groups} groups at random", rng.integers(0, a.groups, nd).astype(np.uint32), (None,))]
            d_rows = torch.zeros(nq * m * 2, dtype=torch.int32, device=dev)
            d_n = torch.zeros(nq, dtype=torch.int32, device=dev)
            d_ng = torch.zeros(nq, dtype=torch.int32, device=dev)
            d_ug = torch.zeros(nq, dtype=torch.int32, device=dev)

        for batch, top, seed in (("head", 10_000, 45), ("mixed", 100_000, 2045), ("tail", nt, 1045)):
            q_ptr, q_terms = synth.make_queries(nq, 3, min(top, nt), seed=seed)
            postings = int(sum((h_bptr[x + 1] - h_bptr[x]) + (h_tptr[x + 1] - h_tptr[x]) for x in q_terms.astype(np.int64)))
            measure(f"{batch}: ss_score_topk k={k}", lambda: sc.score_topk(q_ptr, q_terms, k, out=(d_hits, d_nhits)), lambda med: {"postings": postings})
            facet = measure(f"{batch}: ss_facet_counts totals only", lambda: sc.facet_counts(q_ptr, q_terms, out=(d_match, None, None)),
                            lambda med: {"paper_ms_at_8TBs": round(postings * 4 / HBM * 1e3, 4)})
            for name, group, lds_options in tables:
                sc.set_doc_groups(group)
                n_groups = int(sc.group_values().size)                 # (builds the ranks: no measured call waits for them)
                for lds in lds_options:
                    ctx.set_option("gtopk.lds_groups", lds)
                    out = (d_rows, d_n, d_ng, d_ug, d_match)
                    call = lambda: sc.top_groups(q_ptr, q_terms, 0, m, out=out)      # noqa: E731
                    call()
                    torch.cuda.synchronize()
                    matched = int(d_match.cpu().numpy().view(np.uint32).astype(np.int64).sum())
                    found = int(d_ng.cpu().numpy().view(np.uint32).astype(np.int64).sum())
                    path = "LDS histogram" if lds is None and n_groups <= 8192 else "global atomics"

                    def extra(med):
                        paper = (postings * 4 + matched * 4 + 2 * nq * (n_groups + 2) * 4) / HBM * 1e3
                        return {"over_facet_totals": round(med / facet, 2), "n_groups": n_groups, "matched_docs": matched, "groups_found": found,
                                "paper_ms_at_8TBs": round(paper, 4), "fraction_of_paper": round(paper / med, 3)}
                    measure(f"{batch}: ss_top_groups first 0 m {m}, {name}, {path}", call, extra)
                ctx.set_option("gtopk.lds_groups", None)
        sc.close()
        ti.close()
        bi.close()
    ctx.set_stream(None)
    ctx.close()


if __name__ == "__main__":
    main()
