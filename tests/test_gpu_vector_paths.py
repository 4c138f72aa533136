"""GPU side of the vector path suite: k_vec_topk (csrc/vector.hip) and k_vec_topk_lists (csrc/vector_lists.hip) on the cases of
tests/vector_cases.py, against tests/vector_model.py / tests/vector_lists_model.py.

tests/test_vector_cases_cpu.py shows on the CPU that every case reaches the path it is named for: a list cut inside the round loop
(vec_compact with a real threshold behind it), cuts with every, none and some of the first k slots falling out, a list filled to its
last slot, the per-step check of a tight plan, a block in which some lists are cut and some are not, query blocks behind the first.
Scores are exact 32-bit integers and ties break by doc id, so everything is compared BYTE FOR BYTE, host outputs and device outputs,
on arrays that start from 0xA5 bytes: an entry that must not be written is checked with the ones that must.  No tolerance, no skip.
"""
import functools

import numpy as np
import pytest

from spaghettisearch_amd import engine
from tests import vector_cases as vc
from tests import vector_lists_model as vlm
from tests import vector_model as vm
from tests.test_gpu_collapse import FILL, as_bytes, filled
from tests.test_gpu_score import close_all
from tests.test_gpu_vector import check_topk, tiny_scorer
from tests.test_gpu_vector_lists import check_probed

pytestmark = pytest.mark.gpu

OPTIONS = ("vec.chunk_docs", "vec.list_seg_rows", "vec.list_batch_q")
_ROWS = {}           # case name -> the bytes the device gave


@functools.lru_cache(maxsize=None)
def reference(name):
    """the model's outputs of a case over 0xA5 bytes, computed once and left unchanged"""
    case = vc.get_case(name)
    n_q, k = len(case.qvec), case.k
    hits, n_hits = filled((n_q, k), engine.VEC_HIT_DTYPE), filled(n_q, np.int32)
    if case.kind == "exact":
        return as_bytes(vm.topk(case.qvec, case.vec, k, hits, n_hits, case.mask_id, case.masks))
    return as_bytes(vlm.topk_probed(case.qvec, case.vec, case.cent, case.lod, k, case.n_probe, hits, n_hits, case.mask_id, case.masks))


def run_case(ss_ctx, case):
    """-> the bytes of (hits, n_hits) of the host-output call, after the host and the device form were both held against the model"""
    import torch
    dev = lambda a: torch.from_numpy(a.view(np.uint8) if a.dtype.fields or a.dtype == np.uint32 else a).cuda()      # noqa: E731
    n_q, k = len(case.qvec), case.k
    want = reference(case.name)
    sc, ti, bi = tiny_scorer(ss_ctx, len(case.vec))
    try:
        for name, value in case.options.items():
            ss_ctx.set_option(name, value)
        sc.set_doc_vectors(case.vec)
        if case.masks is not None:
            sc.set_doc_masks(engine.pack_doc_masks(case.masks, len(case.vec)))
        d_q = torch.from_numpy(case.qvec).cuda()
        d_mid = None if case.mask_id is None else torch.from_numpy(case.mask_id).cuda()
        if case.kind == "exact":
            got = check_topk(sc, case.qvec, case.vec, k, case.mask_id, case.masks, tag=case.name)
            d_out = (dev(filled((n_q, k), engine.VEC_HIT_DTYPE)), dev(filled(n_q, np.int32)))
            sc.vector_topk(d_q, k, d_mid, out=d_out)
        else:
            sc.set_vector_lists(case.cent, case.lod)
            got = check_probed(sc, case.qvec, case.vec, case.cent, case.lod, k, case.n_probe, case.mask_id, case.masks, tag=case.name)
            d_out = (dev(filled((n_q, k), engine.VEC_HIT_DTYPE)), dev(filled(n_q, np.int32)), dev(filled((n_q, case.n_probe), np.uint32)))
            sc.vector_topk_probed(d_q, k, case.n_probe, d_mid, out=d_out)
        assert as_bytes(got[:2]) == want[:2], case.name
        assert [t.cpu().numpy().tobytes() for t in d_out] == want, (case.name, "device outputs")
        # a row the call must not write: the empty allow-list, and the entries behind a short row
        n_hits = got[1]
        for q in range(n_q):
            assert got[0][q, n_hits[q]:].tobytes() == bytes([FILL]) * ((k - int(n_hits[q])) * 8), (case.name, q)
        return as_bytes(got[:2])
    finally:
        for name in OPTIONS:
            ss_ctx.set_option(name, None)
        close_all(sc, ti, bi)


@pytest.mark.parametrize("name", vc.CASE_NAMES)
def test_case(ss_ctx, name):
    case = vc.get_case(name)
    rows = _ROWS[name] = run_case(ss_ctx, case)
    if case.same_rows_as:                                      # two chunks / two segments: the bytes the device gave for one
        if case.same_rows_as not in _ROWS:                     # (this case run alone)
            _ROWS[case.same_rows_as] = run_case(ss_ctx, vc.get_case(case.same_rows_as))
        assert rows == _ROWS[case.same_rows_as]
    if name in ("mixed_block", "lists_mixed_block"):
        few, none = (12, 13) if name == "mixed_block" else (17, 18)
        n_hits = np.frombuffer(rows[1], np.int32)
        assert n_hits[few] == 7 and n_hits[none] == 0
