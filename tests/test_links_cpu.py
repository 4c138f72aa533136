"""tests/links_model.py against answers written out by hand, on a graph of 8 nodes with a duplicate edge (0 -> 2 twice), a self-loop
(1 -> 1), a dangling node (4) and a node without in-edges (5); and the ABI's side of the feature without a GPU: the header declares
the three entry points and the ctypes binding holds them."""
import os
import re

import numpy as np

from tests import links_model as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")

ROWS = [[1, 2, 2, 3], [1, 4], [3, 4, 0], [4], [], [4, 0, 3], [4, 7], [6, 4]]
N = len(ROWS)
PTR = np.cumsum([0] + [len(r) for r in ROWS]).astype(np.uint64)
DST = np.array([c for r in ROWS for c in r], dtype=np.uint32)
#                0    1    2    3     4    5    6     7
KEY = np.array([1.0, NAN, 1.0, -0.0, INF, 0.0, -INF, 2.0])


def rows(direction, key, nodes, m):
    links, n_out, degree = lm.top_links(N, PTR, DST, key, direction, nodes, m)
    return [links[i, :n_out[i]].tolist() for i in range(len(nodes))], degree.tolist()


def test_transpose_by_hand():
    assert lm.edge_lists(N, PTR, DST, lm.CHILDREN) == ROWS
    assert lm.edge_lists(N, PTR, DST, lm.PARENTS) == [[2, 5], [0, 1], [0, 0], [0, 2, 5], [1, 2, 3, 5, 6, 7], [], [7], [6]]


def test_parents_with_key():
    got, deg = rows(lm.PARENTS, KEY, list(range(N)), 8)
    assert got == [[2, 5],                 # 1.0 before 0.0
                   [0, 1],                 # the self-loop's node is a candidate of its own row; its NaN key comes last
                   [0],                    # the duplicate edge is one candidate ...
                   [0, 2, 5],              # a tie of 1.0 by id, then 0.0
                   [7, 2, 3, 5, 6, 1],     # 2.0, 1.0, -0.0 = +0.0 by id, -inf, NaN
                   [], [7], [6]]
    assert deg == [2, 2, 2, 3, 6, 0, 1, 1]  # ... and two edges


def test_children_with_key():
    got, deg = rows(lm.CHILDREN, KEY, list(range(N)), 8)
    assert got == [[2, 3, 1], [4, 1], [4, 0, 3], [4], [], [4, 0, 3], [4, 7], [4, 6]]
    assert deg == [4, 2, 3, 1, 0, 3, 2, 2]


def test_without_a_key_ids_ascend():
    got, _ = rows(lm.CHILDREN, None, list(range(N)), 8)
    assert got == [[1, 2, 3], [1, 4], [0, 3, 4], [4], [], [0, 3, 4], [4, 7], [4, 6]]
    got, _ = rows(lm.PARENTS, None, [4, 2, 5], 3)
    assert got == [[1, 2, 3], [0], []]


def test_m_cuts_and_m_above_the_candidates():
    got, deg = rows(lm.PARENTS, KEY, [4, 4, 3], 2)
    assert got == [[7, 2], [7, 2], [0, 2]] and deg == [6, 6, 3]
    links, n_out, _ = lm.top_links(N, PTR, DST, KEY, lm.CHILDREN, [3], 5, links=np.full((1, 5), 77, np.uint32))
    assert n_out.tolist() == [1] and links.tolist() == [[4, 77, 77, 77, 77]]     # entries past n_out are left alone


def test_all_equal_nan_and_infinite_keys():
    assert rows(lm.PARENTS, np.full(N, 3.5), [4], 8)[0] == [[1, 2, 3, 5, 6, 7]]
    assert rows(lm.PARENTS, np.full(N, NAN), [4], 4)[0] == [[1, 2, 3, 5]]
    k = np.array([0.0, -INF, INF, INF, 0.0, -0.0, NAN, -INF])
    assert rows(lm.PARENTS, k, [4], 8)[0] == [[2, 3, 5, 1, 7, 6]]


def test_ids_outside_the_graph_and_the_hits_form():
    got, deg = rows(lm.CHILDREN, KEY, [N, 0xFFFFFFFF, 0], 3)
    assert got == [[], [], [2, 3, 1]] and deg == [0, 0, 4]
    docs = np.array([[0, 5, 9], [4, 4, 4]], dtype=np.uint32)
    links = np.full((2, 3, 2), 99, np.uint32)
    n_out = np.full((2, 3), -7, np.int32)
    degree = np.full((2, 3), 55, np.uint32)
    lm.hit_links(N, PTR, DST, KEY, lm.CHILDREN, docs, [2, 7], 2, links, n_out, degree)      # 7 is clamped to k = 3
    assert links.tolist() == [[[2, 3], [4, 0], [99, 99]], [[99, 99]] * 3]
    assert n_out.tolist() == [[2, 2, -7], [0, 0, 0]] and degree.tolist() == [[4, 3, 55], [0, 0, 0]]


def test_header_and_binding_hold_the_entry_points():
    from spaghettisearch_amd import _lib
    with open(os.path.join(ROOT, "include", "spaghetti_rank.h")) as f:
        header = f.read()
    for name in ("ss_graph_set_link_key", "ss_graph_top_links", "ss_graph_hit_links"):
        assert re.search(r"^int32_t\s+" + name + r"\(", header, re.M), name
        assert name in _lib.PROTOTYPES, name
    assert re.search(r"#define\s+SS_MAX_LINKS\s+64\b", header) and _lib.SS_MAX_LINKS == 64
    assert re.search(r"#define\s+SS_LINKS_PARENTS\s+0\b", header) and re.search(r"#define\s+SS_LINKS_CHILDREN\s+1\b", header)
    assert (_lib.SS_LINKS_PARENTS, _lib.SS_LINKS_CHILDREN) == (lm.PARENTS, lm.CHILDREN) == (0, 1)
    assert re.search(r"#define\s+SS_ABI_VERSION\s+4\b", header)
