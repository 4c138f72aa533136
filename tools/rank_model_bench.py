"""Learned ranking at BASELINE config 3 (10M docs, body table of 640M postings with explain_bench's synthetic positions; the
benchmark's 1024 three-term queries, first token the head term; windows of 100 and 1000 rows, a page of 10; four doc fields), measured
like tools/proximity_bench.py (library on a torch stream shared with the caller, device buffers, blocks of back-to-back calls bracketed
by synchronize), one JSON line per row.  The forests: 100 and 1000 random complete trees of depth 6 (127 nodes each) over the 15
columns of ss_hit_features.  Per window and forest:
  - ss_hit_features alone (proximity entries and query lengths given, no vector scores);
  - ss_rank_model_eval alone on that matrix, under the default "rank.lds_nodes" and with the cap forced to 1, which walks every tree
    from global memory; node visits per second = rows x trees x 7 nodes on a path / time;
  - ss_rerank_hits_by_model as a whole;
  - for scale, ss_rerank_hits_by_proximity on the same rows (code this tool's commit does not touch).
    python tools/rank_model_bench.py [--blocks 6] [--calls 10] [--settle 20] [--docs N]"""
import argparse
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from spaghettisearch_amd import engine, synth  # noqa: E402
from tools.explain_bench import head_term_positions  # noqa: E402

DEPTH = 6


def complete_forest(rng, n_trees, n_features):
    """n_trees complete trees of DEPTH levels of splits in heap order (children 2i + 1, 2i + 2): thresholds near the columns' ranges"""
    n_split, n = (1 << DEPTH) - 1, (1 << (DEPTH + 1)) - 1
    scale = np.array([1, 1, 1, 1, 1000, 4, 4, 50, 1, 8, 1, 1000, 1000, 1000, 1000], dtype=np.float64)
    t = np.zeros((n_trees, n), dtype=engine.TREE_NODE_DTYPE)
    t["feature"][:, n_split:] = -1
    t["value"][:, n_split:] = rng.normal(size=(n_trees, n - n_split)) * 0.01
    f = rng.integers(0, n_features, size=(n_trees, n_split))
    t["feature"][:, :n_split] = f
    t["value"][:, :n_split] = rng.random((n_trees, n_split)) * scale[f]
    t["left"][:, :n_split] = 2 * np.arange(n_split) + 1
    t["right"][:, :n_split] = 2 * np.arange(n_split) + 2
    t["nan_left"][:, :n_split] = rng.integers(0, 2, size=(n_trees, n_split))
    return np.arange(n_trees + 1, dtype=np.uint32) * n, t.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--settle", type=float, default=20.0)           # seconds between building the tables and the first measurement
    ap.add_argument("--docs", type=int, default=10_000_000)          # smaller tables: a rehearsal of the tool, not a measurement
    ap.add_argument("--windows", type=int, nargs="+", default=[100, 1000])
    ap.add_argument("--trees", type=int, nargs="+", default=[100, 1000])
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
        nq, page = 1024, 10
        q_ptr, q_terms = synth.make_queries(nq, 3, min(10_000, nt), seed=45)
        pos_ptr, pos, head_end = head_term_positions(b_term_ptr, n_post, dev)
        bi.set_positions(pos_ptr, pos)
        info = {"n_docs": nd, "n_queries": nq, "page": page}
        del pos
        q_terms = q_terms.copy()
        q_terms[q_ptr[:-1]] = 0                                  # every query's first token: the head term
        sc = engine.Scorer(ctx, ti, bi)
        g = torch.Generator(device=dev)
        g.manual_seed(7)
        sc.set_doc_fields(torch.randint(0, 1000, (4, nd), dtype=torch.int64, device=dev, generator=g))
        qlen = torch.full((nq,), 3, dtype=torch.int32, device=dev)
        rng = np.random.default_rng(5)
        models = {n: engine.RankModel(ctx, engine.RANK_N_FEATURES, complete_forest(rng, n, engine.RANK_N_FEATURES), linear=np.eye(15)[3]) for n in a.trees}
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
            ms = float(np.median(blocks))
            row = {"call": name, "ms_per_batch_median": round(ms, 4), "ms_per_batch_spread": round(float(max(blocks) - min(blocks)), 4),
                   "ms_per_batch_blocks": [round(x, 4) for x in blocks], **info, **extra}
            if "visits" in extra:
                row["node_visits_per_s"] = float(f"{extra['visits'] / (ms * 1e-3):.4g}")
            print(json.dumps(row), flush=True)

        for k_in in a.windows:
            d_hits = torch.empty(nq * k_in * 40, dtype=torch.uint8, device=dev)
            d_nh = torch.empty(nq, dtype=torch.int32, device=dev)
            d_prox = torch.zeros(nq * k_in * 24, dtype=torch.uint8, device=dev)
            d_feat = torch.zeros((nq, k_in, engine.RANK_N_FEATURES), dtype=torch.float64, device=dev)
            d_scores = torch.zeros(nq * k_in, dtype=torch.float64, device=dev)
            o_hits = torch.zeros(nq * page * 40, dtype=torch.uint8, device=dev)
            o_n = torch.zeros(nq, dtype=torch.int32, device=dev)
            o_sc = torch.zeros((nq, page), dtype=torch.float64, device=dev)
            o_px = torch.zeros(nq * page * 24, dtype=torch.uint8, device=dev)
            sc.score_topk(q_ptr, q_terms, k_in, out=(d_hits, d_nh))
            sc.hit_proximity(q_ptr, q_terms, d_hits, d_nh, out=d_prox, k=k_in)
            torch.cuda.synchronize()
            rows = int(d_nh.sum().item())
            extra = {"k_in": k_in, "rows": rows}
            measure("ss_rerank_hits_by_proximity alone (for scale)",
                    lambda: sc.rerank_by_proximity(q_ptr, q_terms, d_hits, d_nh, page, 1.0, 1.0, 0, k_in=k_in, out=(o_hits, o_n, o_sc, o_px)), extra)
            measure("ss_hit_features alone", lambda: sc.hit_features(d_hits, d_nh, d_prox, None, qlen, k_in=k_in, out=d_feat), extra)
            for n_trees, model in models.items():
                ex = {**extra, "trees": n_trees, "visits": nq * k_in * n_trees * (DEPTH + 1)}      # (eval walks every entry of the matrix)
                measure("ss_rank_model_eval alone, default cap", lambda: model.eval(d_feat, out=d_scores), ex)
                with ctx.options(rank__lds_nodes=1):
                    measure("ss_rank_model_eval alone, cap 1 (global path)", lambda: model.eval(d_feat, out=d_scores), ex)
                measure("ss_rerank_hits_by_model",
                        lambda: sc.rerank_by_model(model, d_hits, d_nh, page, d_prox, None, qlen, 0, k_in=k_in, out=(o_hits, o_n, o_sc)),
                        {**extra, "trees": n_trees, "visits": rows * n_trees * (DEPTH + 1)})
        for model in models.values():
            model.close()
        sc.close()
        ti.close()
        bi.close()
    ctx.set_stream(None)
    ctx.close()


if __name__ == "__main__":
    main()
