"""Links of a hit on the benchmark graph (R-MAT, 10M nodes / 50M edges), measured like tools/dedup_bench.py: library on a torch stream
shared with the caller, device buffers throughout, blocks of back-to-back calls bracketed by synchronize; every block is printed.
PageRank row 0 (ten sweeps) is the key.  Rows:
  set_link_key   ss_graph_set_link_key from a device array (an 8 B per node copy on the stream)
  (a)            ss_graph_hit_links on 1024 x 50 hit rows whose docs are uniform random nodes (a text ranking knows nothing of the link
                 graph), parents and children, m = 5 and 64
  (b)            the same with every row the node of the largest in-degree (parents) / out-degree (children): the split path alone
Each row carries the edges its rows hold and the bytes-moved bound: edges x (4 B index + 8 B key gather) at the gather rate of the
sweep's probe on this graph (ss_pr_probe mode 1, uniformly random table rows: edges per second; one cache line per edge there as here).
--sweep repeats (a) and (b) over values of "links.wave_max" / "links.chunk_edges".
    python tools/links_bench.py [--blocks 5] [--calls 10] [--nodes 10000000] [--edges 50000000] [--sweep]"""
import argparse
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from spaghettisearch_amd import _lib, engine, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--nodes", type=int, default=10_000_000)          # (smaller values: a rehearsal of the tool, not a measurement)
    ap.add_argument("--edges", type=int, default=50_000_000)
    ap.add_argument("--sweep", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = engine.Context(0)
    stream = torch.cuda.Stream(device=dev)
    ctx.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        n, e = a.nodes, a.edges
        out_ptr, out_dst = synth.rmat_graph_torch(n, e, seed=42, device=dev)
        g = engine.Graph(ctx, n, out_ptr, out_dst)
        torch.cuda.synchronize()
        gi = g.info()
        indeg = torch.bincount(out_dst.long(), minlength=n)
        outdeg = out_ptr[1:] - out_ptr[:-1]
        hub = {_lib.SS_LINKS_PARENTS: int(indeg.argmax()), _lib.SS_LINKS_CHILDREN: int(outdeg.argmax())}
        print(json.dumps({"row": "graph", "nodes": n, "edges": e, "max_indeg": int(gi.max_indeg), "max_outdeg": int(outdeg.max())}), flush=True)
        rank = torch.zeros(n, dtype=torch.float64, device=dev)
        g.pagerank_dev(0.75, -1.0, [n], rank, max_iter=10)
        # the gather rate the sweep's probe reports (16 topic vectors, uniformly random table rows)
        pr = engine.PageRankState(g, 0.75, -1.0, synth.topic_sizes(n, 16))
        pr.begin()
        probe_ms = [pr.probe(1, 5) for _ in range(3)]
        pr.close()
        edges_per_s = e / (float(np.median(probe_ms)) * 1e-3)
        print(json.dumps({"row": "gather probe (ss_pr_probe mode 1)", "ms": [round(x, 4) for x in probe_ms], "edges_per_s": round(edges_per_s, 0)}), flush=True)
        time.sleep(2.0)                                               # settle after the large allocations

        def blocks_of(call, n_blocks, n_calls):
            for _ in range(2):
                call()
            out = []
            for _ in range(n_blocks):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(n_calls):
                    call()
                torch.cuda.synchronize()
                out.append((time.perf_counter() - t0) / n_calls * 1e3)
            return out
        ms = blocks_of(lambda: g.set_link_key(rank), a.blocks, a.calls)
        print(json.dumps({"row": "set_link_key", "ms_median": round(float(np.median(ms)), 4), "ms_blocks": [round(x, 4) for x in ms],
                          "paper_ms_16B_per_node_at_8TBs": round(n * 16 / 8e12 * 1e3, 4)}), flush=True)
        nq, k = 1024, 50
        rng = np.random.default_rng(7)
        hits = np.zeros((nq, k), dtype=engine.HIT_DTYPE)
        d_n = torch.full((nq,), k, dtype=torch.int32, device=dev)

        def rows(case, d, m, tag):
            hits["doc"] = rng.integers(0, n, size=(nq, k)) if case == "a" else hub[d]
            d_hits = torch.from_numpy(hits.view(np.uint8).reshape(-1)).to(dev)
            out = (torch.zeros(nq * k * m, dtype=torch.int32, device=dev), torch.zeros(nq * k, dtype=torch.int32, device=dev),
                   torch.zeros(nq * k, dtype=torch.int32, device=dev))
            call = lambda: g.hit_links(d_hits, d_n, d, m, out=out, k=k)      # noqa: E731
            heavy = case == "b"
            ms = blocks_of(call, a.blocks, max(1, a.calls // 5) if heavy else a.calls)
            edges_read = int(out[2].long().sum())
            bound = edges_read / edges_per_s * 1e3
            med = float(np.median(ms))
            print(json.dumps({"row": f"({case}) hit_links {'parents' if d == _lib.SS_LINKS_PARENTS else 'children'} m={m}{tag}", "ms_median": round(med, 4),
                              "ms_blocks": [round(x, 4) for x in ms], "edges_read": edges_read, "bytes_moved_12B_per_edge": edges_read * 12,
                              "bound_ms_at_probe_rate": round(bound, 4), "over_bound": round(med / bound, 2) if bound else None,
                              "mean_links": round(float(out[1].float().mean()), 2)}), flush=True)
            return med
        configs = [(None, None)]
        if a.sweep:
            configs = [(256, 256), (512, 512), (1024, 1024), (2048, 2048), (4096, 4096), (256, 1024), (1024, 4096)]
        for wave_max, chunk in configs:
            ctx.set_option("links.wave_max", wave_max)
            ctx.set_option("links.chunk_edges", chunk)
            tag = "" if wave_max is None else f" wave_max={wave_max} chunk_edges={chunk}"
            for m in (5, 64):
                for d in (_lib.SS_LINKS_PARENTS, _lib.SS_LINKS_CHILDREN):
                    t_a = rows("a", d, m, tag)
                    t_b = rows("b", d, m, tag)
                    print(json.dumps({"row": f"(b) / (a) {'parents' if d == _lib.SS_LINKS_PARENTS else 'children'} m={m}{tag}", "ratio": round(t_b / t_a, 1)}), flush=True)
        g.close()
    ctx.set_stream(None)
    ctx.close()


if __name__ == "__main__":
    main()
