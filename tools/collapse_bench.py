"""Collapse by site at BASELINE config 3 (10M docs, 1024 x 3-term OR queries): ms per batch with results in HBM, measured like
tools/mask_bench.py (library on a torch stream shared with the caller, blocks of back-to-back calls bracketed by synchronize).
Rows: (a) ss_score_topk at k = 100; (b) ss_score_topk at k = k_window in {100, 256, 1024}, the scoring a host-side walk would pay
too; (c) ss_score_topk_collapsed at those windows with g = 2, k = 50; (d) ss_collapse_hits alone on the device rows of (b).  The
last lines report (c) - (b), (d), and what the host-side walk has to copy out per batch: k_window rows of 40 bytes per query, with
the time of that device-to-host copy into pinned memory.  Sites: 200 000 of skewed sizes (a tenth of the docs on the largest 0.1 %
of the sites), 2 % of the docs on no site.
    python tools/collapse_bench.py [--blocks 6] [--calls 20]"""
import argparse
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from spaghettisearch_amd import engine, synth  # noqa: E402
from spaghettisearch_amd._lib import SS_NO_GROUP  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--calls", type=int, default=20)
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
        sc = engine.Scorer(ctx, ti, bi)
        rng = np.random.default_rng(7)
        n_sites = max(1, nd // 50)
        group = (n_sites * rng.random(nd) ** 3).astype(np.uint32)      # P(site < x * n_sites) = x^(1/3)
        group[rng.random(nd) < 0.02] = SS_NO_GROUP
        sc.set_doc_groups(group)
        nq, g, k_page = 1024, 2, 50
        q_ptr, q_terms = synth.make_queries(nq, 3, nt // 100, seed=45)
        windows = (100, 256, 1024)
        d_hits = torch.empty(nq * 1024 * 40, dtype=torch.uint8, device=dev)
        d_n = torch.empty(nq, dtype=torch.int32, device=dev)
        d_page = torch.empty(nq * k_page * 40, dtype=torch.uint8, device=dev)
        d_pn = torch.empty(nq, dtype=torch.int32, device=dev)
        d_same = torch.empty(nq * k_page, dtype=torch.int32, device=dev)
        d_kept = torch.empty(nq, dtype=torch.int32, device=dev)
        pinned = torch.empty(nq * 1024 * 40, dtype=torch.uint8).pin_memory()
        page_out = (d_page, d_pn, d_same, d_kept)

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
            print(json.dumps({"row": name, "ms_per_batch_median": round(med, 4), "ms_per_batch_blocks": [round(x, 4) for x in blocks],
                              **extra()}), flush=True)
            return med

        def hits_extra():
            return {"mean_hits_per_query": round(float(d_n.cpu().numpy().mean()), 2)}

        def page_extra():
            return {"mean_page_rows": round(float(d_pn.cpu().numpy().mean()), 2), "mean_kept": round(float(d_kept.cpu().numpy().mean()), 2)}

        measure("(a) score_topk k=100", lambda: sc.score_topk(q_ptr, q_terms, 100, out=(d_hits, d_n)), hits_extra)
        res = {}
        for kw in windows:
            score = measure(f"(b) score_topk k={kw}", lambda: sc.score_topk(q_ptr, q_terms, kw, out=(d_hits, d_n)), hits_extra)
            # (the rows of (b) are still in d_hits / d_n)
            alone = measure(f"(d) collapse_hits alone k_in={kw} g={g} k={k_page}",
                            lambda: sc.collapse_hits(d_hits, d_n, g, k_page, k_in=kw, out=page_out), page_extra)
            fused = measure(f"(c) score_topk_collapsed k_window={kw} g={g} k={k_page}",
                            lambda: sc.score_topk_collapsed(q_ptr, q_terms, kw, g, k_page, out=page_out), page_extra)
            nbytes = nq * kw * 40
            copy = measure(f"copy-out of the window rows k_window={kw} (device to pinned host)",
                           lambda: pinned[:nbytes].copy_(d_hits[:nbytes], non_blocking=True), lambda: {"bytes_per_batch": nbytes})
            res[kw] = (score, fused, alone, copy, nbytes)
        for kw, (score, fused, alone, copy, nbytes) in res.items():
            print(json.dumps({"k_window": kw, "c_minus_b_ms": round(fused - score, 4), "d_ms": round(alone, 4),
                              "host_walk_copy_out_bytes": nbytes, "host_walk_copy_out_ms": round(copy, 4),
                              "page_bytes": nq * k_page * 40}), flush=True)
        sc.close()
        ti.close()
        bi.close()
    ctx.set_stream(None)
    ctx.close()


if __name__ == "__main__":
    main()
