"""Vector lists at 10M docs, dim 128, k 100, 4096 lists, measured like tools/vector_bench.py (library on a torch stream shared with the
caller, device buffers, blocks of back-to-back calls bracketed by synchronize, medians over blocks).  The table is a seeded mixture:
4096 random unit centres, each doc one centre plus noise, quantised to int8 (uniform random int8 has no cluster structure, and recall
on it would say nothing).  The lists come from engine.train_vector_lists on a sample of the table, then ss_vector_assign_lists over
the whole table (timed) and ss_scorer_set_vector_lists (timed).  For n_q in {1, 64, 1024} the exact ss_vector_topk is timed in the same
run, and for n_probe in {1, 8, 32, 128} ss_vector_topk_probed: ms per call, the ratio to the exact call and recall@k against its rows.
    python tools/vector_lists_bench.py [--blocks 5] [--calls 5] [--docs 10000000] [--dim 128] [--k 100] [--lists 4096]"""
import argparse
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from spaghettisearch_amd import engine  # noqa: E402

TINY = (np.array([0, 1], np.uint64), np.array([0], np.uint32), np.array([1.0], np.float32))      # the lexical tables do not matter


def make_scorer(ctx, nd):
    ti, bi = engine.InvertedIndex(ctx, nd, *TINY), engine.InvertedIndex(ctx, nd, *TINY)
    ti.set_weighted(np.ones(nd))
    bi.set_weighted(np.ones(nd))
    return engine.Scorer(ctx, ti, bi), ti, bi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--docs", type=int, default=10_000_000)           # (smaller values: a rehearsal of the tool, not a measurement)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--lists", type=int, default=4096)
    ap.add_argument("--sample", type=int, default=200_000)
    ap.add_argument("--iters", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = engine.Context(0)
    stream = torch.cuda.Stream(device=dev)
    ctx.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        nd, dim, k, n_lists = a.docs, a.dim, a.k, a.lists
        gen = torch.Generator(device=dev).manual_seed(7)
        centres = torch.randn((n_lists, dim), device=dev, generator=gen)
        centres /= centres.norm(dim=1, keepdim=True)

        def mixture(n):                                                   # unit centre + noise of about a third of its length, scaled to int8
            out = torch.empty((n, dim), dtype=torch.int8, device=dev)
            for lo in range(0, n, 1 << 20):
                m = min(1 << 20, n - lo)
                of = torch.randint(0, n_lists, (m,), device=dev, generator=gen)
                x = centres[of] + torch.randn((m, dim), device=dev, generator=gen) * (0.35 / dim ** 0.5)
                out[lo:lo + m] = torch.clamp(torch.round(x * 400.0), -128, 127).to(torch.int8)
            return out
        vec = mixture(nd)
        sc, ti, bi = make_scorer(ctx, nd)
        sc.set_doc_vectors(vec)
        # ---- centroids from a sample, then the whole table assigned and registered
        ns = min(a.sample, nd)
        pick = torch.randperm(nd, device=dev, generator=gen)[:ns]
        sample = vec[pick].cpu().numpy()
        s_sc, s_ti, s_bi = make_scorer(ctx, ns)
        s_sc.set_doc_vectors(sample)
        t0 = time.perf_counter()
        cent, _ = engine.train_vector_lists(s_sc, sample, n_lists, iters=a.iters, seed=9)
        print(json.dumps({"row": f"train_vector_lists sample={ns} lists={n_lists} iters={a.iters}", "s": round(time.perf_counter() - t0, 2)}), flush=True)
        for x in (s_sc, s_ti, s_bi):
            x.close()
        d_cent = torch.from_numpy(cent).to(dev)
        sc.assign_vector_lists(d_cent, device_out=True)                   # warm-up: buffers and LDS attributes
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lists, _ = sc.assign_vector_lists(d_cent, device_out=True)
        torch.cuda.synchronize()
        print(json.dumps({"row": f"ss_vector_assign_lists docs={nd} lists={n_lists}", "ms": round((time.perf_counter() - t0) * 1e3, 2)}), flush=True)
        t0 = time.perf_counter()
        sc.set_vector_lists(d_cent, lists)
        torch.cuda.synchronize()
        sizes = np.bincount(lists.cpu().numpy().view(np.uint32), minlength=n_lists)
        print(json.dumps({"row": f"ss_scorer_set_vector_lists docs={nd} lists={n_lists}", "ms": round((time.perf_counter() - t0) * 1e3, 2),
                          "second_copy_bytes": nd * dim + 4 * nd, "list_len_min": int(sizes.min()), "list_len_median": int(np.median(sizes)),
                          "list_len_max": int(sizes.max())}), flush=True)

        def measure(call):
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
            return float(np.median(blocks)), [round(x, 4) for x in blocks]

        for nq in (1, 64, 1024):
            rows = torch.randint(0, nd, (nq,), device=dev, generator=gen)             # queries: docs of the table under fresh noise
            q = vec[rows].to(torch.float32) + torch.randn((nq, dim), device=dev, generator=gen) * 12.0
            qvec = torch.clamp(torch.round(q), -128, 127).to(torch.int8)
            exact = (torch.empty((nq, k, 2), dtype=torch.int32, device=dev), torch.empty(nq, dtype=torch.int32, device=dev))
            ms_exact, blocks = measure(lambda: sc.vector_topk(qvec, k, out=exact))
            print(json.dumps({"row": f"ss_vector_topk n_q={nq} k={k}", "ms_median": round(ms_exact, 4), "ms_blocks": blocks}), flush=True)
            want = exact[0][:, :, 0].cpu().numpy()
            for n_probe in (1, 8, 32, 128):
                out = (torch.empty((nq, k, 2), dtype=torch.int32, device=dev), torch.zeros(nq, dtype=torch.int32, device=dev))
                ms, blocks = measure(lambda: sc.vector_topk_probed(qvec, k, n_probe, out=out))
                got, n_got = out[0][:, :, 0].cpu().numpy(), out[1].cpu().numpy()
                recall = float(np.mean([len(set(got[i, :n_got[i]].tolist()) & set(want[i].tolist())) / k for i in range(nq)]))
                print(json.dumps({"row": f"ss_vector_topk_probed n_q={nq} k={k} n_probe={n_probe}/{n_lists}", "ms_median": round(ms, 4),
                                  "ms_blocks": blocks, "exact_ms": round(ms_exact, 4), "exact_over_probed": round(ms_exact / ms, 2),
                                  "recall_at_k": round(recall, 4)}), flush=True)
        for x in (sc, ti, bi):
            x.close()
    ctx.set_stream(None)
    ctx.close()


if __name__ == "__main__":
    main()
