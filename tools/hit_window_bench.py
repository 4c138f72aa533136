"""The nine entry points that take a window of result rows, with HOST arrays throughout and with device arrays throughout, on one small
index: the rows the per-feature tools (collapse_bench.py, dedup_bench.py, ...) do not have — those measure device buffers only, and the
staging of host arrays is what csrc/hit_window.hpp holds.  1024 three-term queries; the window is random docs, every count = k_in.
Prints one JSON line per row: the median over the blocks and every block (`ms_per_batch_blocks`: the spread of a row is there to read).
For an A/B against another build of the library: SS_LIB_PATH=<its libspaghetti_rank.so> python tools/hit_window_bench.py.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spaghettisearch_amd import engine, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--docs", type=int, default=1_000_000)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = engine.Context(0)
    stream = torch.cuda.Stream(device=dev)
    ctx.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        nd, nt = a.docs, a.docs // 10
        b = synth.zipf_index_torch(nd, nt, nd * 64, seed=44, device=dev)
        t = synth.zipf_index_torch(nd, nt, nd * 4, seed=144, device=dev)
        bi, ti = engine.InvertedIndex(ctx, nd, *b), engine.InvertedIndex(ctx, nd, *t)
        del b, t
        ti.tfidf_build(nd, False, False, False)
        bi.tfidf_build(nd, False, False, False)
        bi.build_doc_view()
        bi.build_signatures(16)
        sc = engine.Scorer(ctx, ti, bi)
        rng = np.random.default_rng(7)
        sc.set_doc_groups((max(1, nd // 50) * rng.random(nd) ** 3).astype(np.uint32))
        sc.set_doc_fields(rng.integers(0, 1 << 40, (2, nd)).astype(np.int64))
        dim = 128
        sc.set_doc_vectors(torch.randint(-128, 128, (nd, dim), dtype=torch.int8, device=dev))
        nq, k_page, t_stride = 1024, 50, 3
        q_ptr, q_terms = synth.make_queries(nq, 3, nt // 100, seed=45)
        qvec = rng.integers(-128, 128, (nq, dim)).astype(np.int8)

        def measure(name, call):
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
                              "ms_per_batch_blocks": [round(x, 4) for x in blocks]}), flush=True)

        def u8(n):
            return torch.empty(n, dtype=torch.uint8, device=dev)

        def i32(n):
            return torch.empty(n, dtype=torch.int32, device=dev)

        for k_in in (100, 1024):
            hits = np.zeros((nq, k_in), engine.HIT_DTYPE)
            hits["doc"] = rng.integers(0, nd, (nq, k_in))
            n_hits = np.full(nq, k_in, np.int32)
            for where in ("host", "device"):
                if where == "host":
                    h, n, qv = hits, n_hits, qvec
                    page4 = (np.zeros((nq, k_page), engine.HIT_DTYPE), np.zeros(nq, np.int32), np.zeros((nq, k_page), np.uint32), np.zeros(nq, np.int32))
                    vals = np.zeros((nq, k_page), np.int64)
                    scores = np.zeros((nq, k_page), np.int32)
                    o_exp = np.zeros((nq, k_in, t_stride), engine.TERM_MATCH_DTYPE)
                    o_pas = np.zeros((nq, k_in), engine.PASSAGE_DTYPE)
                    o_fld, o_vsc = np.zeros((nq, k_in, 2), np.int64), np.zeros((nq, k_in), np.int32)
                else:
                    h, n, qv = torch.from_numpy(hits.view(np.uint8).reshape(-1)).to(dev), torch.from_numpy(n_hits).to(dev), torch.from_numpy(qvec).to(dev)
                    page4 = (u8(nq * k_page * 40), i32(nq), i32(nq * k_page), i32(nq))
                    vals, scores = torch.empty(nq * k_page, dtype=torch.int64, device=dev), i32(nq * k_page)
                    o_exp, o_pas = u8(nq * k_in * t_stride * 16), u8(nq * k_in * 24)
                    o_fld, o_vsc = torch.empty(nq * k_in * 2, dtype=torch.int64, device=dev), i32(nq * k_in)
                tag = f"k_in={k_in} {where} arrays"
                measure(f"ss_collapse_hits {tag}", lambda: sc.collapse_hits(h, n, 2, k_page, k_in=k_in, out=page4))
                measure(f"ss_score_topk_collapsed k_window={k_in} {where} outputs", lambda: sc.score_topk_collapsed(q_ptr, q_terms, k_in, 2, k_page, out=page4))
                measure(f"ss_dedup_hits {tag}", lambda: sc.dedup_hits(h, n, 8, k_page, k_in=k_in, out=page4))
                measure(f"ss_sort_hits_by_field {tag}", lambda: sc.sort_hits_by_field(h, n, 0, k_page, k_in=k_in, out=(page4[0], page4[1], vals)))
                measure(f"ss_hit_fields {tag}", lambda: sc.hit_fields(h, n, k_in=k_in, out=o_fld))
                measure(f"ss_hit_vector_scores {tag}", lambda: sc.hit_vector_scores(qv, h, n, k_in=k_in, out=o_vsc))
                measure(f"ss_rerank_hits_by_vector {tag}", lambda: sc.rerank_hits_by_vector(qv, h, n, k_page, k_in=k_in, out=(page4[0], page4[1], scores)))
                measure(f"ss_explain_hits {tag}", lambda: sc.explain_hits(q_ptr, q_terms, h, n, t_stride=t_stride, out=o_exp, k=k_in))
                measure(f"ss_best_passages {tag}", lambda: sc.best_passages(q_ptr, q_terms, h, n, out=o_pas, k=k_in))
        sc.close()
        ti.close()
        bi.close()
    ctx.set_stream(None)
    ctx.close()


if __name__ == "__main__":
    main()
