"""Graphs and option sets that more than one PageRank test module uses (test infrastructure)."""
import numpy as np


def csr(n, edges):
    edges = sorted(edges)
    ptr = np.zeros(n + 1, dtype=np.uint64)
    for s, _ in edges:
        ptr[s + 1] += 1
    return np.cumsum(ptr).astype(np.uint64), np.array([d for _, d in edges], dtype=np.uint32)


# the three kernels K <= 2 can run on: k_pr_sweep_n (default), k_pr_sweep padded to 8 topics, k_pr_step
NARROW_VARIANTS = {"wave_items": {}, "padded_8_wide": {"pr__narrow_wave": 0}, "block_items": {"pr__force_narrow": 1}}


def skewed_graph():
    rng = np.random.default_rng(3)
    n = 70000
    edges = {(int(s), 0) for s in range(1, 60001)}                      # hub: 60k in-edges = many W_SEG segments
    edges |= {(int(s), 1) for s in rng.choice(n, 3000, replace=False)}  # several segments at K=1 (128*64 edges each)
    edges |= {(int(s), 2) for s in rng.choice(n, 300, replace=False)}
    edges |= {(int(a), int(b)) for a, b in rng.integers(0, n, size=(50000, 2))}
    return (n,) + csr(n, list(edges))
