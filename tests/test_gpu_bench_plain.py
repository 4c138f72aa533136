"""bench.py without --full: one block of exactly --steps timed steps of the headline and nothing beside it, and --dump-outputs
writes what the timed path computed in its last step — checked against the oracle on the same seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP = 3, 2


def run_bench(out_dir, *args):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
           "--settle", "0", "--dump-outputs", str(out_dir), *args]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    line = json.loads(lines[0])
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["ms_per_step_blocks"]["n_blocks"] == 1
    assert line["ms_per_step"] > 0 and line["higher_is_better"] is True and line["dtype"] == "f64"
    return line


def test_plain_pagerank_run_dumps_the_ranks_of_its_last_sweep(tmp_path, oracle):
    from spaghettisearch_amd import synth
    n, e, kt = 20000, 100000, 16
    line = run_bench(tmp_path, "--nodes", str(n), "--edges", str(e), "--topics", str(kt))
    assert line["metric"] == "pagerank_iters_per_sec" and line["unit"] == "topic-iterations/s"
    assert line["value"] == pytest.approx(kt * 1e3 / line["ms_per_step"], rel=1e-9)
    for key in ("topk", "config2", "cpu_baseline", "pagerank_end_to_end", "pagerank_two_vector_form"):
        assert key not in line, key
    assert sorted(os.listdir(tmp_path)) == ["pagerank_ranks.npy"]
    got = np.load(tmp_path / "pagerank_ranks.npy")
    assert got.dtype == np.float64 and got.shape == (kt, n)          # fewer nodes than the sample size: every column, in order
    out_ptr, out_dst = synth.rmat_graph_torch(n, e, seed=42, device="cuda")
    # begin + the warm-up sweeps + the timed ones
    ref, _ = oracle.pagerank(n, out_ptr.cpu().numpy().view(np.uint64), out_dst.cpu().numpy().view(np.uint32), 0.75, -1.0,
                             synth.topic_sizes(n, kt), max_iter=WARMUP + STEPS)
    np.testing.assert_allclose(got, ref, rtol=1e-9)


def test_plain_topk_run_dumps_the_hits_of_its_last_batch(tmp_path, oracle):
    from spaghettisearch_amd import synth
    nd, nt, bp, tp, nq, k = 200000, 20000, 2000000, 200000, 64, 10
    line = run_bench(tmp_path, "--workload", "topk", "--docs", str(nd), "--terms", str(nt), "--body-postings", str(bp),
                     "--title-postings", str(tp), "--queries", str(nq), "--k", str(k))
    assert line["metric"] == "topk_queries_per_sec" and line["unit"] == "queries/s"
    for key in ("roofline", "tfidf", "tail_queries", "blended_config5", "cpu_baseline"):
        assert key not in line, key
    fields = ("doc", "title", "body", "pagerank", "final")
    assert sorted(os.listdir(tmp_path)) == sorted(f"topk_{f}.npy" for f in fields + ("n_hits",))
    got = {f: np.load(tmp_path / f"topk_{f}.npy") for f in fields + ("n_hits",)}
    assert all(a.dtype == np.float64 for a in got.values())
    b = [x.cpu().numpy() for x in synth.zipf_index_torch(nd, nt, bp, seed=44, device="cuda")]
    t = [x.cpu().numpy() for x in synth.zipf_index_torch(nd, nt, tp, seed=144, device="cuda")]
    b[0], b[1], t[0], t[1] = b[0].view(np.uint64), b[1].view(np.uint32), t[0].view(np.uint64), t[1].view(np.uint32)
    wb, mb, _ = oracle.tfidf(*b, nd, nd)
    wt, mt, _ = oracle.tfidf(*t, nd, nd)
    q_ptr, q_terms = synth.make_queries(nq, 3, min(10_000, nt), seed=45)
    ref, ref_n = oracle.score_topk_batch(nd, (t[0], t[1], wt), (b[0], b[1], wb), mt, mb, q_ptr, q_terms, k)
    assert got["n_hits"].tolist() == ref_n.tolist()
    filled = np.arange(k)[None, :] < ref_n[:, None]
    assert np.array_equal(got["doc"], np.where(filled, ref["doc"], -1))
    for f in fields[1:]:
        np.testing.assert_allclose(got[f], np.where(filled, ref[f], 0), rtol=1e-12, atol=0)
