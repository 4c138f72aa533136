"""Doc fields at BASELINE config 3 (10M docs, 640M body postings, 1024 x 3-term OR queries), measured like tools/dedup_bench.py
(library on a torch stream shared with the caller, device buffers, blocks of back-to-back calls bracketed by synchronize, medians
over blocks).  Rows: (a) ss_doc_field_masks for 1, 16, 256 and 1024 distinct one-clause sets on one field and 256 two-clause sets on
two fields, beside the paper time: column bytes read once per group of 64 sets plus set bytes written, at 8 TB/s; (b) a 1024-query
head batch through ss_score_topk_filtered with 1, 4 and 1024 distinct ranges at about 50 % and 1 % selectivity, beside
ss_score_topk_masked on the same sets registered beforehand; (c) ss_sort_hits_by_field behind 1024 queries at k_in = 100 and 1024,
beside ss_collapse_hits at the same shapes.
    python tools/doc_fields_bench.py [--blocks 6] [--calls 20] [--docs 10000000]"""
import argparse
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from spaghettisearch_amd import engine, synth  # noqa: E402

GROUP = 64          # FM_GROUP of csrc/field.hip


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
        span = 1_000_000
        values = np.stack([rng.integers(0, span, nd), rng.integers(0, span, nd)]).astype(np.int64)
        sc.set_doc_fields(values)
        n_words = (nd + 31) // 32

        def measure(name, call, extra=lambda: {}):
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
            print(json.dumps({"row": name, "ms_median": round(med, 4), "ms_blocks": [round(x, 4) for x in blocks], **extra()}), flush=True)
            return med

        def windows(n, share):
            """n distinct one-clause sets on field 0, each about `share` of the docs"""
            width = int(span * share)
            return [[(0, int(lo), int(lo) + width - 1)] for lo in np.linspace(0, span - width, n).astype(np.int64)]
        # ---- (a) the sets alone
        d_words = torch.empty(1024 * n_words, dtype=torch.int32, device=dev)
        for name, sets, n_fields in [(f"{n} x 1 clause", windows(n, 0.5), 1) for n in (1, 16, 256, 1024)] + \
                                    [("256 x 2 clauses on 2 fields", [w + [(1, 0, span // 2)] for w in windows(256, 0.5)], 2)]:
            ranges = engine.pack_doc_ranges(sets)
            groups = (len(sets) + GROUP - 1) // GROUP
            paper = (groups * n_fields * nd * 8 + len(sets) * n_words * 4) / 8e12 * 1e3
            med = measure(f"(a) ss_doc_field_masks {name}", lambda: sc.doc_field_masks(ranges, out=d_words), lambda: {"paper_ms": round(paper, 4)})
            print(json.dumps({"row": f"(a) {name}: achieved fraction of paper", "fraction": round(paper / med, 3)}), flush=True)
        # ---- (b) filtered scoring beside masked scoring on the same sets, registered beforehand
        nq, k = 1024, 100
        q_ptr, q_terms = synth.make_queries(nq, 3, nt // 100, seed=45)
        d_hits = torch.empty(nq * 1024 * 40, dtype=torch.uint8, device=dev)
        d_n = torch.empty(nq, dtype=torch.int32, device=dev)
        measure("(b) score_topk k=100 (no filter)", lambda: sc.score_topk(q_ptr, q_terms, k, out=(d_hits, d_n)))
        for share in (0.5, 0.01):
            for n_distinct in (1, 4, 1024):
                sets = windows(n_distinct, share)
                which = (np.arange(nq) % n_distinct).astype(np.int32)
                ranges = engine.pack_doc_ranges([sets[i] for i in which])
                tag = f"{n_distinct} distinct ranges of {share:.0%}"
                f_ms = measure(f"(b) score_topk_filtered {tag}", lambda: sc.score_topk_filtered(q_ptr, q_terms, k, ranges=ranges, out=(d_hits, d_n)),
                               lambda: {"mean_hits": round(float(d_n.cpu().numpy().mean()), 2)})
                sc.doc_field_masks(engine.pack_doc_ranges(sets), out=d_words)
                sc.set_doc_masks(d_words[:n_distinct * n_words].view(n_distinct, n_words))
                m_ms = measure(f"(b) score_topk_masked  {tag}", lambda: sc.score_topk_masked(q_ptr, q_terms, which, k, out=(d_hits, d_n)),
                               lambda: {"mean_hits": round(float(d_n.cpu().numpy().mean()), 2)})
                print(json.dumps({"row": f"(b) {tag}: price of building the sets per call", "ms": round(f_ms - m_ms, 4)}), flush=True)
                sc.set_doc_masks(None)
        # ---- (c) the sort behind a scoring batch, beside the collapse kernel of the same shape
        n_sites = max(1, nd // 50)
        sc.set_doc_groups((n_sites * rng.random(nd) ** 3).astype(np.uint32))
        k_page = 50
        page = (torch.empty(nq * k_page * 40, dtype=torch.uint8, device=dev), torch.empty(nq, dtype=torch.int32, device=dev),
                torch.empty(nq * k_page, dtype=torch.int32, device=dev), torch.empty(nq, dtype=torch.int32, device=dev))
        vals = torch.empty(nq * k_page, dtype=torch.int64, device=dev)
        for kw in (100, 1024):
            sc.score_topk(q_ptr, q_terms, kw, out=(d_hits, d_n))
            measure(f"(c) sort_hits_by_field k_in={kw} k={k_page}",
                    lambda: sc.sort_hits_by_field(d_hits, d_n, 0, k_page, descending=True, k_in=kw, out=(page[0], page[1], vals)))
            measure(f"(c) collapse_hits      k_in={kw} g=2 k={k_page}", lambda: sc.collapse_hits(d_hits, d_n, 2, k_page, k_in=kw, out=page))
        sc.close()
        ti.close()
        bi.close()
    ctx.set_stream(None)
    ctx.close()


if __name__ == "__main__":
    main()
