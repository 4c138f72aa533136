"""GPU: the host mirror's late-interaction search (DeviceIndex.SetDocTokens / MaxSimSearch through pybind) on the golden 300 x 80 index
with synthetic token vectors, against the model (tests/maxsim_topk_model.py), by docHash.  The mirror numbers the docs in its own
order, so ties would break differently: the tokens are random over the whole int8 range and the test asserts that no two candidates
of a query score alike, after which the rows are compared exactly."""
import numpy as np
import pytest

from tests import maxsim_topk_model as tm
from tests.test_gpu_host import h, host  # noqa: F401  (module fixture of the host-mirror test)
from tests.test_gpu_host_facet import golden_tables

pytestmark = pytest.mark.gpu

DIM = 64


def test_maxsim_search_equals_the_model(host):
    z, n_docs, n_terms, doc, forw, inv = golden_tables(host)
    di = host.DeviceIndex()
    di.load(forw, inv)
    rng = np.random.default_rng(83)
    m_q = [3, 17, 1, 40]
    qtoks = [rng.integers(-128, 128, (m, DIM)).astype(np.int8) for m in m_q]
    with pytest.raises(RuntimeError, match="SetDocTokens"):
        di.MaxSimSearch([q.tolist() for q in qtoks], 5)
    named = 250                                                              # 0 .. 5 token vectors for the first 250 pages, none for the rest
    counts = np.zeros(n_docs, np.int64)
    counts[:named] = rng.integers(0, 6, named)
    tok_ptr = np.zeros(n_docs + 1, np.uint64)
    tok_ptr[1:] = np.cumsum(counts)
    tok = rng.integers(-128, 128, (int(tok_ptr[-1]), DIM)).astype(np.int8)
    di.SetDocTokens({**{doc[d]: tok[int(tok_ptr[d]):int(tok_ptr[d + 1])].tolist() for d in range(named)}, h("http://nowhere/"): [[1] * DIM]})
    qt_ptr = np.zeros(5, np.uint32)
    qt_ptr[1:] = np.cumsum(m_q)
    qtok = np.concatenate(qtoks)
    some = np.zeros(n_docs, bool)
    some[100:200] = True
    di.SetDocMasks({"some": [doc[i] for i in range(100, 200)]})
    n_cand = int((counts > 0).sum())
    for q in range(4):
        scores = [s for _, s in tm.candidates(qt_ptr, qtok, tok_ptr, tok, q)]
        assert len(scores) == n_cand and len(set(scores)) == n_cand           # no ties: the order does not depend on the numbering
    for k in (1, 20, 300):
        for names, mask_id in (([], None), (["some", "", "some", ""], [0, -1, 0, -1])):
            want = tm.topk(qt_ptr, qtok, tok_ptr, tok, k, np.zeros((4, k), tm.VEC_HIT_DTYPE), np.zeros(4, np.int32), mask_id=mask_id, masks=[some])
            rows = di.MaxSimSearch([q.tolist() for q in qtoks], k, names)
            for q in range(4):
                n = int(want[1][q])
                assert [(r.DocHash, r.Score) for r in rows[q]] == [(doc[int(d)], int(s)) for d, s in want[0][q, :n].tolist()], (k, q)
                assert n == min(k, int((counts[100:200] > 0).sum()) if mask_id and mask_id[q] == 0 else n_cand)
    # a query without tokens scores every candidate 0
    rows = di.MaxSimSearch([[], qtoks[0].tolist()], 400)
    assert len(rows[0]) == n_cand and {r.Score for r in rows[0]} == {0} and {r.DocHash for r in rows[0]} == {doc[d] for d in range(named) if counts[d]}
    with pytest.raises(RuntimeError, match="one mask name per query"):
        di.MaxSimSearch([q.tolist() for q in qtoks], 5, ["some"])
    with pytest.raises(RuntimeError, match="no doc mask named"):
        di.MaxSimSearch([q.tolist() for q in qtoks], 5, ["none", "", "", ""])
    with pytest.raises(RuntimeError, match="wrong length"):
        di.MaxSimSearch([[[1] * 65]], 5)
    with pytest.raises(RuntimeError, match="ss_maxsim_topk"):
        di.MaxSimSearch([[[1] * DIM] * 65], 5)                               # 65 query tokens
    di.SetDocTokens({})
    with pytest.raises(RuntimeError, match="SetDocTokens"):
        di.MaxSimSearch([q.tolist() for q in qtoks], 5)
