"""Term proximity at BASELINE config 3 (10M docs, body table of 640M postings with explain_bench's synthetic positions; the
benchmark's 1024 three-term queries, first token the head term; windows of 100 and 1000 rows, a page of 10), measured like
tools/passage_bench.py (library on a torch stream shared with the caller, device buffers, blocks of back-to-back calls bracketed by
synchronize), one JSON line per row.  Per window:
  - ss_best_passages alone on the window's rows: the yardstick of ss_hit_proximity (the same list searches and the same LDS sort per hit);
  - ss_rerank_hits_by_vector alone (dim 64): with the row above, the yardstick of ss_rerank_hits_by_proximity;
  - ss_hit_proximity alone, ss_rerank_hits_by_proximity alone, ss_score_topk alone and ss_score_topk_proximity.
--yardstick-only runs the first two rows alone: that mode uses nothing this tool's commit added, so the same file runs on the parent
commit's tree (the yardstick of DESIGN.md K4v is taken there, in the same session, after --settle seconds of waiting).
    python tools/proximity_bench.py [--yardstick-only] [--blocks 6] [--calls 10] [--settle 20] [--docs N]"""
import argparse
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from spaghettisearch_amd import engine, synth  # noqa: E402
from tools.explain_bench import head_term_positions  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--yardstick-only", action="store_true")
    ap.add_argument("--settle", type=float, default=20.0)           # seconds between building the tables and the first measurement
    ap.add_argument("--docs", type=int, default=10_000_000)          # smaller tables: a rehearsal of the tool, not a measurement
    ap.add_argument("--windows", type=int, nargs="+", default=[100, 1000])
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = engine.Context(0)
    stream = torch.cuda.Stream(device=dev)
    ctx.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        nd, nt = a.docs, a.docs // 10
        b = synth.zipf_index_torch(nd, nt, nd * 64, seed=44, device=dev)
        t = synth.zipf_index_torch(nd, nt, nd * 4, seed=144, device=dev)
        b_term_ptr, n_post = b[0].clone(), int(b[1].numel())
        bi = engine.InvertedIndex(ctx, nd, *b)
        ti = engine.InvertedIndex(ctx, nd, *t)
        del b, t
        ti.tfidf_build(nd, False, False, False)
        bi.tfidf_build(nd, False, False, False)
        nq, page, dim = 1024, 10, 64
        q_ptr, q_terms = synth.make_queries(nq, 3, min(10_000, nt), seed=45)
        pos_ptr, pos, head_end = head_term_positions(b_term_ptr, n_post, dev)
        bi.set_positions(pos_ptr, pos)
        info = {"n_docs": nd, "n_queries": nq, "page": page, "position_values": int(pos.numel()), "head_term_postings": head_end,
                "yardstick_only": a.yardstick_only}
        del pos
        q_terms = q_terms.copy()
        q_terms[q_ptr[:-1]] = 0                                  # every query's first token: the head term
        sc = engine.Scorer(ctx, ti, bi)
        g = torch.Generator(device=dev)
        g.manual_seed(7)
        sc.set_doc_vectors(torch.randint(-127, 128, (nd, dim), dtype=torch.int8, device=dev, generator=g))
        qvec = torch.randint(-127, 128, (nq, dim), dtype=torch.int8, device=dev, generator=g)
        torch.cuda.synchronize()
        time.sleep(a.settle)

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
            print(json.dumps({"call": name, "ms_per_batch_median": round(float(np.median(blocks)), 4),
                              "ms_per_batch_spread": round(float(max(blocks) - min(blocks)), 4),
                              "ms_per_batch_blocks": [round(x, 4) for x in blocks], **info, **extra}), flush=True)

        for k_in in a.windows:
            d_hits = torch.empty(nq * k_in * 40, dtype=torch.uint8, device=dev)
            d_nh = torch.empty(nq, dtype=torch.int32, device=dev)
            d_pas = torch.zeros(nq * k_in * 24, dtype=torch.uint8, device=dev)
            o_hits = torch.zeros(nq * page * 40, dtype=torch.uint8, device=dev)
            o_n = torch.zeros(nq, dtype=torch.int32, device=dev)
            o_vs = torch.zeros((nq, page), dtype=torch.int32, device=dev)
            sc.score_topk(q_ptr, q_terms, k_in, out=(d_hits, d_nh))
            torch.cuda.synchronize()
            extra = {"k_in": k_in, "rows": int(d_nh.sum().item())}
            measure("ss_best_passages alone (yardstick)", lambda: sc.best_passages(q_ptr, q_terms, d_hits, d_nh, 20, out=d_pas, k=k_in), extra)
            measure("ss_rerank_hits_by_vector alone (yardstick)",
                    lambda: sc.rerank_hits_by_vector(qvec, d_hits, d_nh, page, 0, k_in=k_in, out=(o_hits, o_n, o_vs)), extra)
            if a.yardstick_only:
                continue
            o_sc = torch.zeros((nq, page), dtype=torch.float64, device=dev)
            o_px = torch.zeros(nq * page * 24, dtype=torch.uint8, device=dev)
            measure("ss_hit_proximity alone", lambda: sc.hit_proximity(q_ptr, q_terms, d_hits, d_nh, out=d_pas, k=k_in), extra)
            measure("ss_rerank_hits_by_proximity alone",
                    lambda: sc.rerank_by_proximity(q_ptr, q_terms, d_hits, d_nh, page, 1.0, 1.0, 0, k_in=k_in, out=(o_hits, o_n, o_sc, o_px)), extra)
            measure("ss_score_topk alone", lambda: sc.score_topk(q_ptr, q_terms, k_in, out=(d_hits, d_nh)), extra)
            measure("ss_score_topk_proximity", lambda: sc.score_topk_proximity(q_ptr, q_terms, k_in, page, 1.0, 1.0, 0, out=(o_hits, o_n, o_sc, o_px)),
                    extra)
            torch.cuda.synchronize()
            m = o_px.cpu().numpy().view(engine.PROXIMITY_DTYPE).reshape(nq, page)
            print(json.dumps({"what": "the last page's entries", "k_in": k_in, "with_span": int((m["n_present"] > 0).sum()),
                              "present_histogram": np.bincount(m["n_present"].astype(np.int64).ravel(), minlength=4).tolist()}), flush=True)
        sc.close()
        ti.close()
        bi.close()
    ctx.set_stream(None)
    ctx.close()


if __name__ == "__main__":
    main()
