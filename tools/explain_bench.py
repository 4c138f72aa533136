"""Explain hits at BASELINE config 3 (10M docs, body table of 640M postings; the benchmark's 1024 three-term queries, k = 100),
measured like tools/related_bench.py (library on a torch stream shared with the caller, device buffers, blocks of back-to-back
calls bracketed by synchronize), one JSON line per row:
  - ss_score_topk alone;
  - ss_score_topk followed by ss_explain_hits on its rows: what the new call adds behind the scoring call is the difference;
  - ss_explain_hits alone on rows that are already there;
  - with --positions: the body table gets positional postings (1 - 3 values per posting; every 8th posting of the head term 0 a
    list of 1024 values) and the queries become (0, a, b): the same three rows with long position lists in play;
  - --kernels-only: a short run of the pair alone, for `rocprofv3 --kernel-trace --stats -- python tools/explain_bench.py
    --kernels-only` (k_explain_hits beside k_merge_flat, which does the same searches for the same winners).
    python tools/explain_bench.py [--blocks 6] [--calls 20] [--positions]"""
import argparse
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from spaghettisearch_amd import engine, synth  # noqa: E402


def head_term_positions(term_ptr, n_post, dev):
    """pos_ptr int64[P + 1], pos float32: 1 - 3 values per posting, 1024 for every 8th posting of term 0"""
    idx = torch.arange(n_post, device=dev, dtype=torch.int64)
    lens = 1 + idx % 3
    head_end = int(term_ptr[1].item())
    lens[:head_end:8] = 1024
    pos_ptr = torch.zeros(n_post + 1, dtype=torch.int64, device=dev)
    pos_ptr[1:] = torch.cumsum(lens, dim=0)
    del idx, lens
    g = torch.Generator(device=dev)
    g.manual_seed(46)
    pos = torch.floor(torch.rand(int(pos_ptr[-1].item()), generator=g, device=dev) * 5000.0)
    return pos_ptr, pos, head_end


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--positions", action="store_true")
    ap.add_argument("--kernels-only", action="store_true")
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
        b_term_ptr, n_post = b[0].clone(), int(b[1].numel())
        bi = engine.InvertedIndex(ctx, nd, *b)
        ti = engine.InvertedIndex(ctx, nd, *t)
        del b, t
        ti.tfidf_build(nd, False, False, False)
        bi.tfidf_build(nd, False, False, False)
        nq, k, t_stride = 1024, 100, 3
        q_ptr, q_terms = synth.make_queries(nq, 3, min(10_000, nt), seed=45)
        info = {"n_docs": nd, "n_queries": nq, "k": k, "t_stride": t_stride, "positions": a.positions}
        if a.positions:
            pos_ptr, pos, head_end = head_term_positions(b_term_ptr, n_post, dev)
            bi.set_positions(pos_ptr, pos)
            info.update({"position_values": int(pos.numel()), "head_term_postings": head_end})
            del pos_ptr, pos
            q_terms = q_terms.copy()
            q_terms[q_ptr[:-1]] = 0                              # every query's first token: the head term
        sc = engine.Scorer(ctx, ti, bi)
        d_hits = torch.empty(nq * k * 40, dtype=torch.uint8, device=dev)
        d_nh = torch.empty(nq, dtype=torch.int32, device=dev)
        d_out = torch.zeros(nq * k * t_stride * 16, dtype=torch.uint8, device=dev)

        def score():
            sc.score_topk(q_ptr, q_terms, k, out=(d_hits, d_nh))

        def explain():
            sc.explain_hits(q_ptr, q_terms, d_hits, d_nh, t_stride=t_stride, out=d_out, k=k)

        def pair():
            score()
            explain()

        rows = [("ss_score_topk k=100 + ss_explain_hits, device buffers", pair)]
        if not a.kernels_only:
            rows = [("ss_score_topk k=100, device outputs", score)] + rows + [("ss_explain_hits alone, device buffers", explain)]
        for name, call in rows:
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
                              "ms_per_batch_blocks": [round(x, 4) for x in blocks], **info}), flush=True)
        torch.cuda.synchronize()
        m = d_out.cpu().numpy().view(engine.TERM_MATCH_DTYPE).reshape(nq, k, t_stride)
        n_h = d_nh.cpu().numpy()
        live = np.arange(k)[None, :, None] < n_h[:, None, None]
        flags = m["flags"][np.broadcast_to(live, m.shape)]
        print(json.dumps({"what": "entries of the last call", "written": int(flags.size), "in_title": int((flags & 1).astype(bool).sum()),
                          "in_body": int((flags & 2).astype(bool).sum()), "with_position": int((flags & 4).astype(bool).sum()),
                          "matching_no_table": int(((flags & 3) == 0).sum())}), flush=True)
        sc.close()
        ti.close()
        bi.close()
    ctx.set_stream(None)
    ctx.close()


if __name__ == "__main__":
    main()
