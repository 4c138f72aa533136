"""GPU: the calls that take a window of result rows stage their host arrays through ONE set of scorer-owned device blocks
(csrc/hit_window.hpp).  One scorer, host arrays throughout, entry points taking turns at window widths that make the blocks grow and
cross the kernels' instance cut (128 rows): every result equals, byte for byte, what the Python model gives for that call alone.  Then
an all-device chain (collapse into explain) with a host-array call between its two steps equals the chain alone.  Every comparison is
tobytes() on whole output arrays that start from 0xA5 bytes, so an entry a call must not write is checked with the ones it must."""
import numpy as np
import pytest

from spaghettisearch_amd import engine
from tests import collapse_model as cm
from tests import doc_fields_model as fm
from tests.test_gpu_collapse import as_bytes, filled, outputs, random_rows
from tests.test_gpu_collapse import world  # noqa: F401  (module fixture: the golden 300 x 80 tables and a group table)
from tests.test_gpu_doc_fields import field_table, sort_outputs
from tests.test_gpu_explain import model as explain_model, prefilled, queries
from tests.test_gpu_score import close_all, make_scorer

pytestmark = pytest.mark.gpu

N_Q, SMALL, LARGE, T_STRIDE = 3, 5, 130, 4
UNKNOWN = 0xFFFFFFFF


def test_entry_points_take_turns_at_the_shared_blocks(ss_ctx, world):  # noqa: F811
    import torch
    n_docs, group = world["n_docs"], world["group"]
    rng = np.random.default_rng(130)
    values = field_table(rng, n_docs)[:3]
    q_ptr, q_terms = queries([[3], [0, 1, 2, 70], [79, UNKNOWN, 1]])
    sc, ti, bi = make_scorer(ss_ctx, n_docs, world["title"], world["body"], world["mt"], world["mb"])
    try:
        sc.set_doc_groups(group)
        sc.set_doc_fields(values)
        small, n_small = random_rows(rng, N_Q, SMALL, n_docs + 5), np.array([SMALL, 0, 3], np.int32)
        large, n_large = random_rows(rng, N_Q, LARGE, n_docs + 5), np.array([LARGE, 1, 129], np.int32)

        def collapse_small():
            got = sc.collapse_hits(small, n_small, 1, SMALL, out=outputs(N_Q, SMALL))
            assert as_bytes(got) == as_bytes(cm.collapse(small, n_small, group, 1, 0, SMALL, *outputs(N_Q, SMALL)))

        def sort_large():
            got = sc.sort_hits_by_field(large, n_large, 1, LARGE, descending=True, first=2, out=sort_outputs(N_Q, LARGE))
            assert as_bytes(got) == as_bytes(fm.sort_page(large, n_large, values, n_docs, 1, True, 2, LARGE, *sort_outputs(N_Q, LARGE)))

        collapse_small()
        sort_large()                                                          # the blocks grow; the four-wave instance
        got = sc.hit_fields(small, n_small, out=filled((N_Q, SMALL, 3), np.int64))
        assert got.tobytes() == fm.gather(small, n_small, values, n_docs, filled((N_Q, SMALL, 3), np.int64)).tobytes()
        got = sc.explain_hits(q_ptr, q_terms, large, n_large, t_stride=T_STRIDE, out=prefilled(N_Q, LARGE, T_STRIDE))
        assert got.tobytes() == explain_model(world, q_ptr, q_terms, large, n_large, T_STRIDE, body_pos=None).tobytes()
        collapse_small()

        # ---- an all-device chain, collapse into explain: alone, then with a host-array call between its two steps
        lib = ss_ctx.lib
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()      # noqa: E731
        d_rows, d_n = dev(large), dev(n_large)

        def chain(between):
            d_page, d_pn = dev(filled((N_Q, LARGE), engine.HIT_DTYPE)), dev(filled(N_Q, np.int32))
            d_out = dev(prefilled(N_Q, LARGE, T_STRIDE))
            torch.cuda.synchronize()
            assert lib.ss_collapse_hits(sc.h, N_Q, LARGE, d_rows.data_ptr(), d_n.data_ptr(), 2, 0, LARGE, d_page.data_ptr(), d_pn.data_ptr(),
                                        None, None) == 0
            if between:
                sort_large()
            assert lib.ss_explain_hits(sc.h, N_Q, q_ptr.ctypes.data, q_terms.ctypes.data, LARGE, d_page.data_ptr(), d_pn.data_ptr(), T_STRIDE,
                                       d_out.data_ptr()) == 0
            ss_ctx.synchronize()
            return [t.cpu().numpy().tobytes() for t in (d_page, d_pn, d_out)]

        alone = chain(False)
        assert chain(True) == alone
        page = cm.collapse(large, n_large, group, 2, 0, LARGE, filled((N_Q, LARGE), engine.HIT_DTYPE), filled(N_Q, np.int32))
        assert alone[:2] == as_bytes(page[:2])
        assert alone[2] == explain_model(world, q_ptr, q_terms, page[0], page[1], T_STRIDE, body_pos=None).tobytes()
    finally:
        close_all(sc, ti, bi)
