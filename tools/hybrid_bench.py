"""Hybrid search at BASELINE config 3 (10M docs, body table of 640M postings, the benchmark's 1024 three-term queries) with one int8
vector of dim 128 per doc, measured like tools/vector_bench.py (library on a torch stream shared with the caller, device buffers,
blocks of back-to-back calls bracketed by synchronize, medians over blocks behind 3 warm-up calls), one JSON line per row:
  (1) ss_score_docs at k_in = 100 and 1024 on random docs, beside the bytes it must touch at 8 TB/s (per (doc, token, field) one
      64-byte line of records and one 4-byte weight line, per doc two magnitudes and the 40-byte row) and ss_explain_hits at the same
      shapes on the same build, which does the same searches without the sums;
  (2) ss_fuse_hits at (k_lex, k_vec) = (100, 100) and (1024, 1024), for disjoint and for identical lists, beside
      ss_rerank_hits_by_vector at k_in = 100 / 1024, the nearest existing window call;
  (3) ss_hybrid_topk at k_window = 100 beside ss_score_topk_masked at k = 100, ss_vector_topk at k = 100 and ss_fuse_hits on their
      rows, each measured alone in the same run, and the sum of the three.
    python tools/hybrid_bench.py [--blocks 5] [--calls 5] [--docs 10000000] [--dim 128] [--settle 8]"""
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
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--settle", type=float, default=8.0)              # seconds of idle in front of the first GPU call, as bench.py
    a = ap.parse_args()
    if a.settle > 0 and a.docs >= 10_000_000:
        time.sleep(a.settle)
    dev = torch.device("cuda", 0)
    ctx = engine.Context(0)
    stream = torch.cuda.Stream(device=dev)
    ctx.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        nd, nt, dim = a.docs, a.docs // 10, a.dim
        b = synth.zipf_index_torch(nd, nt, nd * 64, seed=44, device=dev)
        t = synth.zipf_index_torch(nd, nt, nd * 4, seed=144, device=dev)
        bi = engine.InvertedIndex(ctx, nd, *b)
        ti = engine.InvertedIndex(ctx, nd, *t)
        del b, t
        ti.tfidf_build(nd, False, False, False)
        bi.tfidf_build(nd, False, False, False)
        sc = engine.Scorer(ctx, ti, bi)
        gen = torch.Generator(device=dev).manual_seed(7)
        vec = torch.randint(-128, 128, (nd, dim), dtype=torch.int8, device=dev, generator=gen)
        sc.set_doc_vectors(vec)
        del vec
        nq, n_tok = 1024, 3
        q_ptr, q_terms = synth.make_queries(nq, n_tok, min(10_000, nt), seed=45)
        qvec = torch.randint(-128, 128, (nq, dim), dtype=torch.int8, device=dev, generator=gen)
        rng = np.random.default_rng(8)

        def measure(name, call, extra=None):
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
            print(json.dumps({"row": name, "ms_median": round(med, 4), "ms_blocks": [round(x, 4) for x in blocks], **(extra(med) if extra else {})}),
                  flush=True)
            return med

        def rows_of(docs):
            hits = np.zeros(docs.shape, engine.HIT_DTYPE)
            hits["doc"] = docs
            hits["final"] = rng.random(docs.shape)
            return torch.from_numpy(hits.view(np.uint8).reshape(-1)).to(dev)

        def page_out(k):
            return (torch.empty(nq * k * 40, dtype=torch.uint8, device=dev), torch.empty(nq, dtype=torch.int32, device=dev),
                    torch.empty(nq * k * 16, dtype=torch.uint8, device=dev), torch.empty(nq, dtype=torch.int32, device=dev))

        # ---- (1) the rows of given docs
        for k_in in (100, 1024):
            docs = rng.integers(0, nd, (nq, k_in)).astype(np.uint32)
            d_docs = torch.from_numpy(docs.view(np.int32)).to(dev)
            d_n = torch.full((nq,), k_in, dtype=torch.int32, device=dev)
            d_rows = torch.empty(nq * k_in * 40, dtype=torch.uint8, device=dev)
            touch_ms = nq * k_in * (2 * n_tok * (64 + 64) + 2 * 8 + 4 + 40) / HBM * 1e3
            med = measure(f"(1) ss_score_docs n_q={nq} k_in={k_in}", lambda: sc.score_docs(q_ptr, q_terms, d_docs, d_n, out=d_rows),
                          lambda m: {"touched_bytes_at_8TBs_ms": round(touch_ms, 5), "ratio": round(m / touch_ms, 1)})
            d_hits = rows_of(docs)
            d_exp = torch.empty(nq * k_in * n_tok * 16, dtype=torch.uint8, device=dev)
            measure(f"(1) ss_explain_hits n_q={nq} k={k_in} (the same searches, no sums)",
                    lambda: sc.explain_hits(q_ptr, q_terms, d_hits, d_n, t_stride=n_tok, out=d_exp, k=k_in),
                    lambda m: {"score_docs_over_explain": round(med / m, 2)})
            del d_docs, d_rows, d_hits, d_exp

        # ---- (2) the fusion of given lists
        k_page = 50
        for k_w in (100, 1024):
            d_n = torch.full((nq,), k_w, dtype=torch.int32, device=dev)
            both = np.stack([rng.choice(nd, 2 * k_w, replace=False) for _ in range(nq)]).astype(np.uint32)
            out = page_out(k_page)
            meds = {}
            for kind in ("disjoint", "identical"):
                lex_docs = both[:, :k_w]
                vec_docs = both[:, k_w:] if kind == "disjoint" else np.ascontiguousarray(both[:, :k_w][:, ::-1])
                d_lex = rows_of(lex_docs)
                vh = np.zeros((nq, k_w), engine.VEC_HIT_DTYPE)
                vh["doc"], vh["score"] = vec_docs, rng.integers(-2 ** 20, 2 ** 20, (nq, k_w))
                d_vec = torch.from_numpy(vh.view(np.int32).reshape(nq, k_w, 2)).to(dev)
                for mode, name in ((engine.FUSE_RRF, "rrf"), (engine.FUSE_WEIGHTED, "weighted")):
                    meds[(kind, name)] = measure(
                        f"(2) ss_fuse_hits n_q={nq} k_lex=k_vec={k_w} k={k_page} {kind} {name}",
                        lambda: sc.fuse_hits(q_ptr, q_terms, qvec, d_lex, d_n, d_vec, d_n, k_page, mode=mode, w_vec=1e-4, k_lex=k_w, k_vec=k_w,
                                             out=out))
            d_lex = rows_of(both[:, :k_w])
            rr_out = (out[0], out[1], torch.empty(nq * k_page, dtype=torch.int32, device=dev))
            measure(f"(2) ss_rerank_hits_by_vector n_q={nq} k_in={k_w} k={k_page}",
                    lambda: sc.rerank_hits_by_vector(qvec, d_lex, d_n, k_page, k_in=k_w, out=rr_out),
                    lambda m: {"fuse_over_rerank": {f"{kd} {nm}": round(v / m, 2) for (kd, nm), v in meds.items()}})

        # ---- (3) the one-call form beside its three parts
        k_w = 100
        lex_out = (torch.empty(nq * k_w * 40, dtype=torch.uint8, device=dev), torch.empty(nq, dtype=torch.int32, device=dev))
        vec_out = (torch.empty((nq, k_w, 2), dtype=torch.int32, device=dev), torch.empty(nq, dtype=torch.int32, device=dev))
        out = page_out(k_page)
        m_lex = measure(f"(3) ss_score_topk_masked n_q={nq} k={k_w}", lambda: sc.score_topk_masked(q_ptr, q_terms, None, k_w, out=lex_out))
        m_vec = measure(f"(3) ss_vector_topk n_q={nq} k={k_w}", lambda: sc.vector_topk(qvec, k_w, out=vec_out))
        m_fuse = measure(f"(3) ss_fuse_hits on their rows k={k_page} rrf",
                         lambda: sc.fuse_hits(q_ptr, q_terms, qvec, lex_out[0], lex_out[1], vec_out[0], vec_out[1], k_page, k_lex=k_w, k_vec=k_w,
                                              out=out))
        total = m_lex + m_vec + m_fuse
        measure(f"(3) ss_hybrid_topk n_q={nq} k_window={k_w} k={k_page} rrf", lambda: sc.hybrid_topk(q_ptr, q_terms, qvec, k_w, k_page, out=out),
                lambda m: {"sum_of_the_three_ms": round(total, 4), "hybrid_over_sum": round(m / total, 3)})
        torch.cuda.synchronize()
        print(json.dumps({"what": "the last ss_hybrid_topk", "mean_union": round(float(out[3].float().mean()), 1),
                          "mean_rows": round(float(out[1].float().mean()), 1)}), flush=True)
        sc.close()
        ti.close()
        bi.close()
    ctx.set_stream(None)
    ctx.close()


if __name__ == "__main__":
    main()
