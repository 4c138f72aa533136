"""ctypes binding of libspaghetti_rank.so (the C ABI in include/spaghetti_rank.h).

There is no CPU fallback: if the shared library is missing the import of the
product API fails loudly, and without a gfx950 device ``ss_init`` fails.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SS_LIB_PATH") or os.path.join(_HERE, "libspaghetti_rank.so")   # SS_LIB_PATH: A/B builds

SS_OK = 0
SS_MAX_TOPK = 1024
SS_MAX_TOPICS = 64
SS_MAX_QUERY_TERMS = 64
SS_MAX_FEEDBACK_DOCS = 64
SS_UNKNOWN_TERM = 0xFFFFFFFF
SS_NO_GROUP = 0xFFFFFFFF
SS_MAX_WORD_BYTES = 64
SS_MAX_EDIT_DIST = 3
SS_MAX_SUGGEST = 64
SS_MAX_COMPLETE = 64
SS_MAX_SIG_SLOTS = 32
SS_SIG_EMPTY = 0xFFFFFFFF
SS_MAX_LINKS = 64
SS_LINKS_PARENTS = 0
SS_LINKS_CHILDREN = 1
SS_MAX_DOC_FIELDS = 4
SS_MAX_RANGE_CLAUSES = 4
SS_NO_FIELD_VALUE = -(2 ** 63)
SS_MAX_VEC_DIM = 1024
SS_NO_VEC_SCORE = -(2 ** 31)
SS_DIV_WEIGHT_MAX = 65536
SS_MAX_VEC_LISTS = 65536
SS_NO_LIST = 0xFFFFFFFF
SS_FUSE_RRF = 0
SS_FUSE_WEIGHTED = 1

ERR_NAMES = {0: "SS_OK", 1: "SS_ERR_INVALID", 2: "SS_ERR_NO_DEVICE", 3: "SS_ERR_HIP", 4: "SS_ERR_OOM",
             5: "SS_ERR_UNSORTED", 6: "SS_ERR_STATE", 7: "SS_ERR_UNSUPPORTED", 8: "SS_ERR_COMM"}
SS_COMM_ID_BYTES = 128


class SpaghettiError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{ERR_NAMES.get(code, code)}: {msg}")
        self.code = code


class SsHit(C.Structure):
    _fields_ = [("doc", C.c_uint32), ("_pad", C.c_uint32), ("title", C.c_double), ("body", C.c_double),
                ("pagerank", C.c_double), ("final", C.c_double)]


class SsTermMatch(C.Structure):
    _fields_ = [("title_w", C.c_float), ("body_w", C.c_float), ("flags", C.c_uint32), ("body_pos", C.c_float)]


class SsPassage(C.Structure):
    _fields_ = [("start", C.c_float), ("last", C.c_float), ("n_distinct", C.c_uint32), ("n_occ", C.c_uint32), ("token_mask", C.c_uint64)]


class SsProximity(C.Structure):
    _fields_ = [("start", C.c_float), ("end", C.c_float), ("n_present", C.c_uint32), ("n_occ", C.c_uint32), ("token_mask", C.c_uint64)]


class SsDocRange(C.Structure):
    _fields_ = [("field", C.c_int32), ("_pad", C.c_int32), ("lo", C.c_int64), ("hi", C.c_int64)]


class SsVecHit(C.Structure):
    _fields_ = [("doc", C.c_uint32), ("score", C.c_int32)]


class SsDivInfo(C.Structure):
    _fields_ = [("rel", C.c_int32), ("sim", C.c_int32)]


class SsFuseParams(C.Structure):
    _fields_ = [("mode", C.c_int32), ("rrf_c", C.c_int32), ("w_lex", C.c_double), ("w_vec", C.c_double)]


class SsFused(C.Structure):
    _fields_ = [("score", C.c_double), ("vec_score", C.c_int32), ("lex_rank", C.c_uint16), ("vec_rank", C.c_uint16)]


class SsGraphInfo(C.Structure):
    _fields_ = [("n_nodes", C.c_uint64), ("n_edges", C.c_uint64), ("n_nondangling", C.c_uint64),
                ("n_rows_local", C.c_uint64), ("n_edges_local", C.c_uint64), ("max_indeg", C.c_uint32),
                ("rank", C.c_int32), ("world", C.c_int32)]


_vp = C.c_void_p
_i32 = C.c_int32
_u64 = C.c_uint64
_f64 = C.c_double

# name -> (restype, argtypes); every symbol include/spaghetti_rank.h declares
PROTOTYPES = {
    "ss_abi_version": (_i32, []),
    "ss_init": (_i32, [_i32, C.POINTER(_vp)]),
    "ss_shutdown": (_i32, [_vp]),
    "ss_set_stream": (_i32, [_vp, _vp]),
    "ss_synchronize": (_i32, [_vp]),
    "ss_set_option": (_i32, [_vp, C.c_char_p, C.c_int64]),
    "ss_last_error": (C.c_char_p, [_vp]),
    "ss_comm_unique_id": (_i32, [_vp]),
    "ss_comm_init": (_i32, [_vp, _vp, _i32, _i32]),
    "ss_comm_split": (_i32, [_vp, _i32, _i32]),
    "ss_comm_destroy": (_i32, [_vp]),
    "ss_comm_info": (_i32, [_vp, C.POINTER(_i32), C.POINTER(_i32)]),
    "ss_comm_allreduce_u64": (_i32, [_vp, _vp, _u64]),
    "ss_comm_allgather": (_i32, [_vp, _vp, _vp, _u64]),
    "ss_graph_create": (_i32, [_vp, _u64, _u64, _vp, _vp, _i32, _i32, C.POINTER(_vp)]),
    "ss_graph_apply_delta": (_i32, [_vp, _u64, _u64, _vp, _vp, _vp]),
    "ss_graph_get_info": (_i32, [_vp, C.POINTER(SsGraphInfo)]),
    "ss_graph_destroy": (_i32, [_vp]),
    "ss_graph_set_link_key": (_i32, [_vp, _vp]),
    "ss_graph_top_links": (_i32, [_vp, _i32, _u64, _vp, _i32, _vp, _vp, _vp]),
    "ss_graph_hit_links": (_i32, [_vp, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _vp]),
    "ss_pagerank_run": (_i32, [_vp, _f64, _f64, _i32, _i32, _vp, _vp, _vp]),
    "ss_pr_create": (_i32, [_vp, _f64, _f64, _i32, _i32, _vp, C.POINTER(_vp)]),
    "ss_pr_destroy": (_i32, [_vp]),
    "ss_pr_set_teleport": (_i32, [_vp, _vp, _vp]),
    "ss_pr_begin": (_i32, [_vp]),
    "ss_pr_step": (_i32, [_vp, _i32]),
    "ss_pr_lean_sweeps": (_i32, [_vp, C.POINTER(C.c_int64)]),
    "ss_pr_finalize": (_i32, [_vp]),
    "ss_pr_exchange_buffers": (_i32, [_vp, C.POINTER(_vp), C.POINTER(_u64), C.POINTER(_vp), C.POINTER(_u64)]),
    "ss_pr_exchange": (_i32, [_vp, _i32]),
    "ss_pagerank_run_sharded": (_i32, [_vp, _f64, _f64, _i32, _i32, _vp, _i32, _vp, _vp, _vp]),
    "ss_pagerank_run_group": (_i32, [_vp, _i32, _f64, _f64, _i32, _i32, _vp, _vp, _vp]),
    "ss_pr_status": (_i32, [_vp, _vp, C.POINTER(_i32), C.POINTER(_i32), _vp, _vp]),
    "ss_pr_read_local": (_i32, [_vp, _vp, _vp]),
    "ss_pr_read": (_i32, [_vp, _vp]),
    "ss_pr_probe": (_i32, [_vp, _i32, _i32, C.POINTER(C.c_float)]),
    "ss_index_create": (_i32, [_vp, _u64, _u64, _vp, _vp, _vp, C.POINTER(_vp)]),
    "ss_index_destroy": (_i32, [_vp]),
    "ss_tfidf_build": (_i32, [_vp, _u64, _vp, _vp, _vp]),
    "ss_index_apply_delta": (_i32, [_vp, _u64, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _vp]),
    "ss_index_apply_delta_pos": (_i32, [_vp, _u64, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp]),
    "ss_index_resize": (_i32, [_vp, _u64, _u64]),
    "ss_index_read_magnitudes": (_i32, [_vp, _u64, _vp, _vp]),
    "ss_index_refresh_magnitudes": (_i32, [_vp, _vp]),
    "ss_index_get_info": (_i32, [_vp, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64)]),
    "ss_index_read": (_i32, [_vp, _vp, _vp, _vp]),
    "ss_index_read_positions": (_i32, [_vp, _vp, _vp]),
    "ss_index_set_doc_freq": (_i32, [_vp, _vp]),
    "ss_index_set_weighted": (_i32, [_vp, _vp]),
    "ss_index_set_positions": (_i32, [_vp, _vp, _vp]),
    "ss_index_build_doc_view": (_i32, [_vp]),
    "ss_index_drop_doc_view": (_i32, [_vp]),
    "ss_index_read_doc_view": (_i32, [_vp, _vp, _vp, _vp]),
    "ss_index_doc_top_terms": (_i32, [_vp, _u64, _vp, _i32, _vp, _vp, _vp]),
    "ss_scorer_create": (_i32, [_vp, _vp, _vp, C.POINTER(_vp)]),
    "ss_scorer_destroy": (_i32, [_vp]),
    "ss_scorer_set_prior": (_i32, [_vp, _i32, _vp]),
    "ss_score_topk": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp]),
    "ss_score_topk_phrase": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp]),
    "ss_score_topk_submit": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp]),
    "ss_score_topk_collect": (_i32, [_vp, C.c_uint64, _vp, _vp]),
    "ss_scorer_set_doc_masks": (_i32, [_vp, _i32, _vp]),
    "ss_score_topk_masked": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp]),
    "ss_score_topk_constrained": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp]),
    "ss_similar_topk": (_i32, [_vp, _i32, _vp, _i32, _vp, _vp, _i32, _vp, _vp]),
    "ss_related_terms": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp]),
    "ss_explain_hits": (_i32, [_vp, _i32, _vp, _vp, _i32, _vp, _vp, _i32, _vp]),
    "ss_best_passages": (_i32, [_vp, _i32, _vp, _vp, _i32, _vp, _vp, _i32, _vp]),
    "ss_hit_proximity": (_i32, [_vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp]),
    "ss_rerank_hits_by_proximity": (_i32, [_vp, _i32, _vp, _vp, _i32, _vp, _vp, C.c_double, C.c_double, _i32, _i32, _vp, _vp, _vp, _vp]),
    "ss_score_topk_proximity": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, C.c_double, C.c_double, _i32, _i32, _vp, _vp, _vp, _vp]),
    "ss_rank_model_create": (_i32, [_vp, _i32, _vp, C.c_double, _i32, _vp, _vp, C.POINTER(_vp)]),
    "ss_rank_model_destroy": (_i32, [_vp]),
    "ss_rank_model_get_info": (_i32, [_vp, _vp]),
    "ss_rank_model_eval": (_i32, [_vp, C.c_int64, _vp, _vp]),
    "ss_hit_features": (_i32, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ss_rerank_hits_by_model": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp]),
    "ss_scorer_set_doc_groups": (_i32, [_vp, _vp]),
    "ss_collapse_hits": (_i32, [_vp, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "ss_score_topk_collapsed": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "ss_index_build_signatures": (_i32, [_vp, _i32]),
    "ss_index_drop_signatures": (_i32, [_vp]),
    "ss_index_read_signatures": (_i32, [_vp, _u64, _vp, _vp, C.POINTER(_i32)]),
    "ss_dedup_hits": (_i32, [_vp, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "ss_scorer_set_doc_fields": (_i32, [_vp, _i32, _vp]),
    "ss_doc_field_masks": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp]),
    "ss_score_topk_filtered": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp]),
    "ss_facet_counts": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    "ss_field_topk": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "ss_scorer_group_values": (_i32, [_vp, _vp, _vp]),
    "ss_top_groups": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "ss_field_stats": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp]),
    "ss_field_histogram": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, C.c_int64, C.c_uint64, _vp, _i32, _vp, _vp]),
    "ss_sort_hits_by_field": (_i32, [_vp, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "ss_hit_fields": (_i32, [_vp, _i32, _i32, _vp, _vp, _vp]),
    "ss_scorer_set_doc_vectors": (_i32, [_vp, _i32, _vp]),
    "ss_vector_topk": (_i32, [_vp, _i32, _vp, _vp, _i32, _vp, _vp]),
    "ss_hit_vector_scores": (_i32, [_vp, _i32, _vp, _i32, _vp, _vp, _vp]),
    "ss_rerank_hits_by_vector": (_i32, [_vp, _i32, _vp, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp]),
    "ss_scorer_set_doc_tokens": (_i32, [_vp, _i32, _vp, _vp]),
    "ss_hit_maxsim_scores": (_i32, [_vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp]),
    "ss_rerank_hits_by_maxsim": (_i32, [_vp, _i32, _vp, _vp, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp]),
    "ss_maxsim_topk": (_i32, [_vp, _i32, _vp, _vp, _vp, _i32, _vp, _vp]),
    "ss_diversify_hits": (_i32, [_vp, _i32, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "ss_scorer_set_vector_lists": (_i32, [_vp, _i32, _vp, _vp]),
    "ss_vector_assign_lists": (_i32, [_vp, _i32, _vp, _vp, _vp]),
    "ss_vector_topk_probed": (_i32, [_vp, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp]),
    "ss_score_docs": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp]),
    "ss_fuse_hits": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp]),
    "ss_hybrid_topk": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp]),
    "ss_lexicon_create": (_i32, [_vp, _u64, _vp, _vp, _vp, C.POINTER(_vp)]),
    "ss_lexicon_set_freq": (_i32, [_vp, _vp]),
    "ss_lexicon_get_info": (_i32, [_vp, C.POINTER(_u64), C.POINTER(_u64)]),
    "ss_lexicon_read_order": (_i32, [_vp, _vp]),
    "ss_lexicon_destroy": (_i32, [_vp]),
    "ss_lexicon_prefix": (_i32, [_vp, _i32, _vp, _vp, C.c_int64, _i32, _vp, _vp, _vp]),
    "ss_lexicon_suggest": (_i32, [_vp, _i32, _vp, _vp, _i32, C.c_uint32, _i32, _vp, _vp, _vp]),
    "ss_lexicon_complete": (_i32, [_vp, _i32, _vp, _vp, C.c_uint32, _i32, _vp, _vp, _vp, _vp]),
    "ss_merge_hits": (_i32, [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "ss_last_kernel_ms": (_i32, [_vp, _i32, C.POINTER(C.c_float)]),
}

ABI_VERSION = 4   # SS_ABI_VERSION of include/spaghetti_rank.h this binding follows (tests/test_abi.py compares the two)
_lib = None


def load() -> C.CDLL:
    """Load the shared library and attach prototypes.  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(make -C spaghettisearch_amd/csrc). There is no CPU fallback.")
    # One HIP runtime per process: torch bundles its own libamdhip64.so.7 / libhsa-runtime64.so.1.
    # If this library pulled in /opt/rocm's copy first, a later `import torch` would bring up a
    # second runtime in the same process ("no ROCm-capable device"), and torch streams / device
    # pointers could not be shared with the library.  Importing torch first makes the dynamic
    # loader resolve our libamdhip64.so.7 dependency to the copy torch already mapped.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)   # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    if lib.ss_abi_version() != ABI_VERSION:
        raise ImportError(f"{LIB_PATH}: ABI version {lib.ss_abi_version()}, this binding was written for {ABI_VERSION} "
                          "(include/spaghetti_rank.h: SS_ABI_VERSION) - rebuild the library")
    _lib = lib
    return lib


def check(rc: int, ctx=None) -> None:
    if rc != SS_OK:
        msg = load().ss_last_error(ctx)
        raise SpaghettiError(rc, msg.decode("utf-8", "replace") if msg else "")
