"""Word completions at the benchmark's sizes: the 1M-word Zipf vocabulary of tools/lexicon_bench.py, 1024 prefixes per batch, m = 10,
device buffers, measured like tools/lexicon_bench.py (library on a torch stream shared with the caller, blocks of back-to-back calls
bracketed by synchronize, after the settle wait bench.py uses).  ONE row per process run, one JSON line:
  --row complete   ss_lexicon_complete for --prefixes one | two | four (bytes per prefix; four = the first four bytes of vocabulary
                   words, so every prefix matches) | empty (the worst case: 1024 empty prefixes) with --queries prefixes per batch
                   (1 = one user alone); --parts forces "lexicon.complete_parts".  The row
                   carries the bytes of the frequencies inside the ranges (4 B per match), the yardstick of a stream.
  --row prefix     ss_lexicon_prefix on the same prefixes, k = 50: the yardstick (run from a checkout of the parent commit as well:
                   the row uses nothing newer).
  --row copy       the copy rate of the box: a device-to-device copy of --copy-mib MiB, read + written bytes per second.
  --row hostsort   what a caller had to do before: page the whole range of every prefix back to the host (ss_lexicon_prefix, host
                   buffers, k = 1024 per page) and sort it there by freq (numpy lexsort); one batch per timed step.
    python tools/complete_bench.py --row complete --prefixes two [--queries 1024] [--parts 4] [--vocab-cache FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))
from spaghettisearch_amd import engine  # noqa: E402
from lexicon_bench import vocabulary  # noqa: E402


def load_vocabulary(n, cache):
    """-> (ptr uint64 [n + 1], bytes uint8); the cache file only saves the minute the generator takes"""
    if cache and os.path.exists(cache):
        z = np.load(cache)
        if int(z["ptr"].shape[0]) == n + 1:
            return z["ptr"], z["data"]
    words = vocabulary(n, seed=71)
    ptr = np.zeros(n + 1, dtype=np.uint64)
    ptr[1:] = np.cumsum([len(w) for w in words])
    data = np.frombuffer(b"".join(words), dtype=np.uint8).copy()
    if cache:
        np.savez(cache, ptr=ptr, data=data)
    return ptr, data


def make_prefixes(kind, nq, ptr, data):
    rng = np.random.default_rng(74)
    if kind == "empty":
        return [b""] * nq
    if kind == "four":
        ids = rng.integers(0, ptr.shape[0] - 1, nq)
        return [bytes(data[int(ptr[t]):int(ptr[t]) + 4]) for t in ids]
    return [bytes(r) for r in rng.integers(97, 123, (nq, {"one": 1, "two": 2}[kind]), dtype=np.uint8)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--row", choices=["complete", "prefix", "copy", "hostsort"], required=True)
    ap.add_argument("--prefixes", choices=["one", "two", "four", "empty"], default="two")
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--parts", type=int, default=0)
    ap.add_argument("--m", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--terms", type=int, default=1_000_000)           # smaller: a rehearsal of the tool, not a measurement
    ap.add_argument("--settle", type=float, default=8.0)
    ap.add_argument("--copy-mib", type=int, default=1024)
    ap.add_argument("--vocab-cache", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)

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
        return {"ms_per_batch_median": round(float(np.median(blocks)), 4), "ms_per_batch_blocks": [round(x, 4) for x in blocks]}

    if a.row == "copy":
        if a.settle > 0:
            time.sleep(a.settle)
        src = torch.zeros(a.copy_mib << 20, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        r = measure(lambda: dst.copy_(src))
        rate = 2 * (a.copy_mib << 20) / (r["ms_per_batch_median"] * 1e-3)
        print(json.dumps({"call": f"device-to-device copy of {a.copy_mib} MiB", **r, "read_plus_written_bytes_per_s": float(f"{rate:.4g}")}), flush=True)
        return
    ptr, data = load_vocabulary(a.terms, a.vocab_cache)
    freq = (np.random.default_rng(72).zipf(1.3, a.terms) % (1 << 20)).astype(np.uint32) + 1
    prefixes = make_prefixes(a.prefixes, a.queries, ptr, data)
    if a.settle > 0:
        time.sleep(a.settle)
    ctx = engine.Context(0)
    stream = torch.cuda.Stream(device=dev)
    ctx.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        lx = engine.Lexicon(ctx, (ptr, data), freq)
        nq, m, k = a.queries, a.m, 50
        info = {"n_terms": a.terms, "n_queries": nq, "prefixes": a.prefixes}
        p_terms = torch.zeros(nq * k, dtype=torch.int32, device=dev)
        p_n = torch.zeros(nq, dtype=torch.int32, device=dev)
        p_match = torch.zeros(nq, dtype=torch.int64, device=dev)
        lx.prefix(prefixes, k, 0, out=(p_terms, p_n, p_match))
        torch.cuda.synchronize()
        n_match = p_match.cpu().numpy()
        info["matches_per_prefix_mean"] = round(float(n_match.mean()), 1)
        info["freq_bytes_in_ranges"] = int(n_match.sum()) * 4
        if a.row == "prefix":
            print(json.dumps({"call": f"ss_lexicon_prefix k={k}, device buffers", **measure(lambda: lx.prefix(prefixes, k, 0, out=(p_terms, p_n, p_match))),
                              **info}), flush=True)
        elif a.row == "complete":
            ctx.set_option("lexicon.complete_parts", a.parts or None)
            c_terms = torch.zeros(nq * m, dtype=torch.int32, device=dev)
            c_freq = torch.zeros(nq * m, dtype=torch.int32, device=dev)
            c_n = torch.zeros(nq, dtype=torch.int32, device=dev)
            c_match = torch.zeros(nq, dtype=torch.int64, device=dev)
            r = measure(lambda: lx.complete(prefixes, m, 1, out=(c_terms, c_freq, c_n, c_match)))
            torch.cuda.synchronize()
            # the rows of the last call against numpy on the host: a wrong row must not be timed as a right one
            od = lx.order()
            got_t, got_n = c_terms.cpu().numpy().view(np.uint32).reshape(nq, m), c_n.cpu().numpy()
            lb = np.zeros(nq, dtype=np.int64)
            for q in range(min(nq, 16)):
                rows, _, _ = lx.prefix([prefixes[q]], 1)
                if n_match[q]:
                    lb[q] = int(np.nonzero(od == rows[0, 0])[0][0])
                    ids = od[lb[q]:lb[q] + int(n_match[q])]
                    best = ids[np.argsort(-freq[ids].astype(np.int64), kind="stable")][:m]
                    assert got_n[q] == len(best) and (got_t[q, :got_n[q]] == best).all(), f"row {q} differs from the host's"
            print(json.dumps({"call": f"ss_lexicon_complete m={m} min_freq=1, device buffers", **r, **info,
                              "complete_parts": a.parts or "default"}), flush=True)
        else:
            def host_sort():
                for pre in prefixes:
                    ids, first = [], 0
                    while True:
                        terms, n_out, total = lx.prefix([pre], 1024, first)
                        ids.append(terms[0, :n_out[0]])
                        first += 1024
                        if first >= int(total[0]):
                            break
                    ids = np.concatenate(ids)
                    ids[np.argsort(-freq[ids].astype(np.int64), kind="stable")][:m]
            a.calls, a.blocks = 1, 3
            print(json.dumps({"call": f"ss_lexicon_prefix pages of 1024 to the host + numpy sort by freq, m={m}", **measure(host_sort), **info}), flush=True)
        lx.close()
    ctx.set_stream(None)
    ctx.close()


if __name__ == "__main__":
    main()
