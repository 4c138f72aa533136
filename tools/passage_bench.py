"""Best passages at BASELINE config 3 (10M docs, body table of 640M postings; the benchmark's 1024 three-term queries, k = 100,
width 20), measured like tools/explain_bench.py (library on a torch stream shared with the caller, device buffers, blocks of
back-to-back calls bracketed by synchronize), one JSON line per row.  With --positions (the measurement: without it the body table
has no positional postings and every entry is zero) the body table gets explain_bench's positional postings (1 - 3 values per
posting; every 8th posting of the head term 0 a list of 1024 values) and the queries become (0, a, b):
  - ss_score_topk alone;
  - ss_score_topk followed by ss_best_passages on its rows: what the new call adds behind the scoring call is the difference;
  - ss_best_passages alone on rows that are already there;
  - ss_explain_hits alone on the same rows: the yardstick;
  - the share of written entries whose position values exceed "passage.lds_events" (--lds-events sets it), i.e. that took the
    global-memory path, counted from the tables on the device;
  - --kernels-only: a short run of the pair alone, for `rocprofv3 --kernel-trace --stats -- python tools/passage_bench.py
    --positions --kernels-only`.
    python tools/passage_bench.py --positions [--blocks 6] [--calls 20] [--lds-events N]"""
import argparse
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from spaghettisearch_amd import engine, synth  # noqa: E402
from tools.explain_bench import head_term_positions  # noqa: E402


def values_per_entry(term_ptr, post_doc, pos_ptr, q_ptr, q_terms, docs, n_h):
    """[n_q][k] int64: position values under the query's distinct terms for every hit (0 behind n_hits), as the kernel counts them"""
    n_q, k = docs.shape
    total = torch.zeros((n_q, k), dtype=torch.int64, device=docs.device)
    for q in range(n_q):
        d = docs[q].to(torch.int64)
        for t in sorted(set(int(x) for x in q_terms[q_ptr[q]:q_ptr[q + 1]])):
            if t + 1 >= term_ptr.numel():
                continue
            lo, hi = int(term_ptr[t].item()), int(term_ptr[t + 1].item())
            if hi == lo:
                continue
            seg = post_doc[lo:hi].to(torch.int64)
            x = torch.searchsorted(seg, d).clamp(max=hi - lo - 1)
            found = seg[x] == d
            total[q] += torch.where(found, pos_ptr[lo + x + 1] - pos_ptr[lo + x], torch.zeros_like(x))
    live = torch.arange(k, device=docs.device)[None, :] < n_h[:, None]
    return torch.where(live, total, torch.zeros_like(total)), live


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--positions", action="store_true")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--width", type=int, default=20)
    ap.add_argument("--lds-events", type=int, action="append")      # more than one: the passage rows are repeated per value
    ap.add_argument("--docs", type=int, default=10_000_000)          # smaller tables: a rehearsal of the tool, not a measurement
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = engine.Context(0)
    stream = torch.cuda.Stream(device=dev)
    ctx.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        nd, nt = a.docs, a.docs // 10
        b = synth.zipf_index_torch(nd, nt, nd * 64, seed=44, device=dev)
        t = synth.zipf_index_torch(nd, nt, nd * 4, seed=144, device=dev)
        b_term_ptr, b_doc, n_post = b[0].clone(), b[1].clone(), int(b[1].numel())
        bi = engine.InvertedIndex(ctx, nd, *b)
        ti = engine.InvertedIndex(ctx, nd, *t)
        del b, t
        ti.tfidf_build(nd, False, False, False)
        bi.tfidf_build(nd, False, False, False)
        nq, k, t_stride = 1024, 100, 3
        q_ptr, q_terms = synth.make_queries(nq, 3, min(10_000, nt), seed=45)
        info = {"n_docs": nd, "n_queries": nq, "k": k, "width": a.width, "positions": a.positions}
        pos_ptr = torch.zeros(n_post + 1, dtype=torch.int64, device=dev)
        if a.positions:
            pos_ptr, pos, head_end = head_term_positions(b_term_ptr, n_post, dev)
            bi.set_positions(pos_ptr, pos)
            info.update({"position_values": int(pos.numel()), "head_term_postings": head_end})
            del pos
            q_terms = q_terms.copy()
            q_terms[q_ptr[:-1]] = 0                              # every query's first token: the head term
        sc = engine.Scorer(ctx, ti, bi)
        d_hits = torch.empty(nq * k * 40, dtype=torch.uint8, device=dev)
        d_nh = torch.empty(nq, dtype=torch.int32, device=dev)
        d_out = torch.zeros(nq * k * 24, dtype=torch.uint8, device=dev)
        d_exp = torch.zeros(nq * k * t_stride * 16, dtype=torch.uint8, device=dev)

        def score():
            sc.score_topk(q_ptr, q_terms, k, out=(d_hits, d_nh))

        def passage():
            sc.best_passages(q_ptr, q_terms, d_hits, d_nh, a.width, out=d_out, k=k)

        def explain():
            sc.explain_hits(q_ptr, q_terms, d_hits, d_nh, t_stride=t_stride, out=d_exp, k=k)

        def pair():
            score()
            passage()

        def measure(name, call, extra):
            for _ in range(3):
                call()
            blocks = []
            for _ in range(1 if a.kernels_only else a.blocks):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    call()
                torch.cuda.synchronize()
                blocks.append((time.perf_counter() - t0) / a.calls * 1e3)
            print(json.dumps({"call": name, "ms_per_batch_median": round(float(np.median(blocks)), 4),
                              "ms_per_batch_blocks": [round(x, 4) for x in blocks], **info, **extra}), flush=True)

        score()
        if not a.kernels_only:
            measure("ss_score_topk k=100, device outputs", score, {})
            measure("ss_explain_hits alone, device buffers", explain, {})
        torch.cuda.synchronize()
        docs = d_hits.view(torch.int32).reshape(nq, k, 10)[:, :, 0].contiguous()
        n_vals, live = values_per_entry(b_term_ptr, b_doc, pos_ptr, q_ptr, q_terms, docs, d_nh)
        written = int(live.sum().item())
        for cap in a.lds_events or [None]:
            ctx.set_option("passage.lds_events", cap)
            eff = 512 if cap is None else min(max(cap, 1), 4096)
            extra = {"lds_events": eff, "entries_written": written, "entries_on_the_long_path": int((n_vals > eff).sum().item()),
                     "long_path_share": round(float((n_vals > eff).sum().item()) / max(written, 1), 4),
                     "values_per_entry_max": int(n_vals.max().item())}
            measure("ss_score_topk k=100 + ss_best_passages, device buffers", pair, extra)
            if not a.kernels_only:
                measure("ss_best_passages alone, device buffers", passage, extra)
        ctx.set_option("passage.lds_events", None)
        torch.cuda.synchronize()
        m = d_out.cpu().numpy().view(engine.PASSAGE_DTYPE).reshape(nq, k)[live.cpu().numpy()]
        print(json.dumps({"what": "entries of the last call", "written": int(m.size), "with_passage": int((m["n_occ"] > 0).sum()),
                          "distinct_terms_histogram": np.bincount(m["n_distinct"].astype(np.int64), minlength=4).tolist(),
                          "occurrences_max": int(m["n_occ"].max()) if m.size else 0}), flush=True)
        sc.close()
        ti.close()
        bi.close()
    ctx.set_stream(None)
    ctx.close()


if __name__ == "__main__":
    main()
