"""Term lexicon at the benchmark's sizes: a synthetic vocabulary of 1M distinct words (lengths 3 .. 14 over a - z, Zipf freq) and
1024 misspelt query words (a vocabulary word with one random edit), measured like tools/passage_bench.py (library on a torch stream
shared with the caller, device buffers, blocks of back-to-back calls bracketed by synchronize, after the settle wait bench.py uses),
one JSON line per row:
  - ss_lexicon_suggest at max_dist 1 and 2, m = 10, for every --chunk value ("lexicon.chunk_terms"; none = the default alone):
    ms per batch and word comparisons per second (a comparison = one (query word, vocabulary word) pair of the length groups the
    call reads);
  - ss_lexicon_prefix for 1024 two-byte prefixes, k = 50;
  - ss_lexicon_create (host sort + upload), once;
  - with --yardstick-docs N > 0: the same process's ss_score_topk tail batch (1024 three-term OR queries, term ranks uniform over
    the vocabulary of an N-doc index, k = 50, device outputs): the only yardstick of scale.
    python tools/lexicon_bench.py [--blocks 6] [--calls 20] [--chunk 1024 --chunk 4096 --chunk 16384] [--yardstick-docs 10000000]"""
import argparse
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from spaghettisearch_amd import engine, synth  # noqa: E402


def vocabulary(n, seed):
    """n distinct words, lengths 3 .. 14 (most at 6 .. 9), ids in random order -> list of bytes"""
    rng = np.random.default_rng(seed)
    share = np.array([0.005, 0.03, 0.08, 0.14, 0.17, 0.17, 0.14, 0.10, 0.07, 0.05, 0.03, 0.015])
    words = set()
    while len(words) < n:
        for L, s in zip(range(3, 15), share / share.sum()):
            rows = rng.integers(97, 123, (int((n - len(words)) * s * 1.05) + 8, L), dtype=np.uint8)
            words.update(bytes(r) for r in rows)
    words = sorted(words)[:n]
    return [words[i] for i in rng.permutation(n)]


def misspell(words, n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for w in (words[i] for i in rng.integers(0, len(words), n)):
        b, op, i = bytearray(w), int(rng.integers(0, 4)), int(rng.integers(0, len(w) - 1))
        if op == 0:
            b[i] = 97 + (b[i] - 97 + 1 + int(rng.integers(0, 25))) % 26
        elif op == 1:
            b[i], b[i + 1] = b[i + 1], b[i]
        elif op == 2:
            del b[i]
        else:
            b.insert(i, int(rng.integers(97, 123)))
        out.append(bytes(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--terms", type=int, default=1_000_000)           # smaller: a rehearsal of the tool, not a measurement
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--chunk", type=int, action="append")             # more than one: the suggest rows are repeated per value
    ap.add_argument("--settle", type=float, default=8.0)
    ap.add_argument("--yardstick-docs", type=int, default=0)
    a = ap.parse_args()
    words = vocabulary(a.terms, seed=71)
    freq = (np.random.default_rng(72).zipf(1.3, a.terms) % (1 << 20)).astype(np.uint32) + 1
    queries = misspell(words, a.queries, seed=73)
    lens = np.array([len(w) for w in words])
    count = np.bincount(lens, minlength=66)
    compared = {d: int(sum(count[max(len(q) - d, 0):len(q) + d + 1].sum() for q in queries)) for d in (1, 2)}
    ptr = np.zeros(a.terms + 1, dtype=np.uint64)
    ptr[1:] = np.cumsum(lens)
    data = np.frombuffer(b"".join(words), dtype=np.uint8).copy()
    if a.settle > 0:
        time.sleep(a.settle)
    dev = torch.device("cuda", 0)
    ctx = engine.Context(0)
    stream = torch.cuda.Stream(device=dev)
    ctx.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        t0 = time.perf_counter()
        lx = engine.Lexicon(ctx, (ptr, data), freq)
        info = {"n_terms": a.terms, "n_bytes": int(ptr[-1]), "n_queries": a.queries}
        print(json.dumps({"call": "ss_lexicon_create (host sort, grouping, upload)", "ms": round((time.perf_counter() - t0) * 1e3, 1), **info}), flush=True)
        nq, m, k = a.queries, 10, 50
        d_terms = torch.zeros(nq * m, dtype=torch.int32, device=dev)
        d_dist = torch.zeros(nq * m, dtype=torch.int32, device=dev)
        d_n = torch.zeros(nq, dtype=torch.int32, device=dev)
        p_terms = torch.zeros(nq * k, dtype=torch.int32, device=dev)
        p_n = torch.zeros(nq, dtype=torch.int32, device=dev)
        p_match = torch.zeros(nq, dtype=torch.int64, device=dev)
        rng = np.random.default_rng(74)
        prefixes = [bytes(r) for r in rng.integers(97, 123, (nq, 2), dtype=np.uint8)]

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
            row = {"call": name, "ms_per_batch_median": round(med, 4), "ms_per_batch_blocks": [round(x, 4) for x in blocks], **info, **extra}
            if "word_comparisons" in extra:
                row["word_comparisons_per_s"] = float(f"{extra['word_comparisons'] / (med * 1e-3):.4g}")
            print(json.dumps(row), flush=True)

        for chunk in a.chunk or [None]:
            ctx.set_option("lexicon.chunk_terms", chunk)
            for d in (1, 2):
                measure(f"ss_lexicon_suggest max_dist={d} m={m}, device buffers",
                        lambda d=d: lx.suggest(queries, d, m, 1, out=(d_terms, d_dist, d_n)),
                        {"chunk_terms": 4096 if chunk is None else chunk, "word_comparisons": compared[d]})
        ctx.set_option("lexicon.chunk_terms", None)
        torch.cuda.synchronize()
        n = d_n.cpu().numpy()
        print(json.dumps({"what": "rows of the last suggest call", "rows_with_a_suggestion": int((n > 0).sum()), "rows_full": int((n == m).sum()),
                          "mean_row_length": round(float(n.mean()), 2)}), flush=True)
        measure(f"ss_lexicon_prefix two-byte prefixes k={k}, device buffers", lambda: lx.prefix(prefixes, k, 0, out=(p_terms, p_n, p_match)), {})
        torch.cuda.synchronize()
        print(json.dumps({"what": "matches per two-byte prefix", "mean": round(float(p_match.cpu().numpy().mean()), 1)}), flush=True)
        lx.close()
        if a.yardstick_docs > 0:
            nd, nt = a.yardstick_docs, a.yardstick_docs // 10
            b = synth.zipf_index_torch(nd, nt, nd * 64, seed=44, device=dev)
            t = synth.zipf_index_torch(nd, nt, nd * 4, seed=144, device=dev)
            bi = engine.InvertedIndex(ctx, nd, *b)
            ti = engine.InvertedIndex(ctx, nd, *t)
            del b, t
            ti.tfidf_build(nd, False, False, False)
            bi.tfidf_build(nd, False, False, False)
            sc = engine.Scorer(ctx, ti, bi)
            q_ptr, q_terms = synth.make_queries(nq, 3, nt, seed=45)
            d_hits = torch.empty(nq * k * 40, dtype=torch.uint8, device=dev)
            d_nh = torch.empty(nq, dtype=torch.int32, device=dev)
            info = {"n_docs": nd, "n_queries": nq}
            measure(f"ss_score_topk tail batch (term ranks U[1,{nt}]) k={k}, device outputs: the yardstick",
                    lambda: sc.score_topk(q_ptr, q_terms, k, out=(d_hits, d_nh)), {})
            sc.close()
            ti.close()
            bi.close()
    ctx.set_stream(None)
    ctx.close()


if __name__ == "__main__":
    main()
