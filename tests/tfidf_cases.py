"""Tables built to reach the partition paths of the TF-IDF build (csrc/tfidf.hip, csrc/tfidf_plan.hpp), and a model that says which they reach.

No GPU and no library here: numpy only.

  * Builders.  Every case is (name, n_docs, term_ptr, post_doc, tf, total_docs, options, expect_paths).  `options` holds the library
    options the case runs under ("tfidf.*") and, for a table that stands for one doc-range shard, "df_extra": per term the number of
    postings the term has on other shards (df_global = local length + df_extra).  `expect_paths` names the paths the case is
    built for.
  * paths(n_docs, term_ptr, post_doc, options): a plain restatement of the HOST arithmetic of csrc/tfidf_plan.hpp (geometry():
    shift, bucket count, block ranges, head threshold; tests/test_tfidf_plan_cpu.py holds it against the header) and of the head level, plus a walk over the chunks of every block that follows the
    control flow of k_scatter<true> (head ranges, head-only chunks, the term window and where it starts).  It computes no weight and
    no magnitude: expectations come from the oracle alone.
  * value_paths(...): which float32 edges the ORACLE's results of a case show (zero / denormal / overflowing squares, idf <= 0).
  * expected(case, tfidf): the oracle's results of the first and the second build of a case (whole-corpus table for shard cases).
  * exactness(...): are the float64 sums of a case's float32 squares exact, whatever their order?

tests/test_tfidf_cases_cpu.py proves every claim on the CPU; tests/test_gpu_tfidf_paths.py runs the kernels on the same tables.
"""
import functools
from collections import namedtuple
from fractions import Fraction

import numpy as np

# ---- the constants of csrc/tfidf_plan.hpp the model relies on (test_tfidf_cases_cpu.py holds them against the ones the header's
# ---- harness prints) ------------------------------------------------------------------------------------------------------------
CH = 4096                 # postings per chunk of k_weight_count (and k_weight)
SC_CH = 8192              # postings per chunk of k_scatter
SC_TPB = 1024             # threads of a k_scatter block (one probe of the coarse window search each)
SC_PT = SC_CH // SC_TPB   # consecutive postings per thread
SC_WIN = SC_CH            # most window entries staged per chunk
SC_PF = 1024              # largest window the prefetch takes
NB_MAX = 4096
SC_BPT_MAX = NB_MAX // SC_TPB   # most buckets an owner thread of k_scatter keeps cursors for
HEAD_CAP = 1024
HEAD_LEVELS = 24
HEAD_PIECE = 2048

Case = namedtuple("Case", "name n_docs term_ptr post_doc tf total_docs options expect_paths")


def lib_options(options):
    return {k: int(v) for k, v in options.items() if k.startswith("tfidf.")}


# ---------------------------------------------------------------------------------------------------------------------------------
# the path model

def _div_up(a, b):
    return -(-a // b)


def geometry(n_docs, n_post, options):
    """make_plan of csrc/tfidf_plan.hpp, restated.  The fields behind "bucketed" exist for bucketed tables only."""
    o = lib_options(options)
    N, P = int(n_docs), int(n_post)
    shift = max(10, min(14, o.get("tfidf.bucket_shift", 13)))
    forced = (N >> shift) >= NB_MAX
    if forced:
        shift = 14
    nb = _div_up(max(N, 1), 1 << shift)
    min_p = o.get("tfidf.bucket_min", 1 << 22) % (1 << 64)       # the library reads the option as uint64: a negative value is a huge one
    g = {"shift": shift, "shift_forced": forced, "nb": nb,
         "bucketed": P >= max(min_p, 1) and P < (1 << 32) and nb <= NB_MAX}
    if not g["bucketed"]:
        return g
    unit = max(SC_CH, CH)
    blocks = max(1, o.get("tfidf.blocks", 4096))
    per = max(unit, _div_up(_div_up(P, blocks), unit) * unit)
    min_run = o.get("tfidf.head_min_run", 64)
    bpt, nbt = (_div_up(nb, SC_TPB) + 1) & ~1, (nb + 1) & ~1
    g.update(per=per, nblk=_div_up(P, per), bpt=bpt, nbt=nbt,
             head_thr=max(min_run * nb, 2 * unit + 1) if min_run > 0 else 0,
             bpt_inst=2 if bpt <= 2 else 4 if bpt <= 4 else SC_BPT_MAX, too_many_buckets=bpt > SC_BPT_MAX,
             scatter_lds_bytes=SC_CH * 8 + nbt * 8 + 64, bucket_lds_bytes=(1 << shift) * 8 + (3 * HEAD_CAP + 4) * 4)
    return g


def head_selection(lens, thr):
    """k_head_hist / k_head_select / k_head_sort -> (level j, head term ids ascending, clamped?)."""
    if not thr:
        return 0, np.zeros(0, np.int64), False
    hist = [int((lens >= (thr << j)).sum()) for j in range(HEAD_LEVELS)]
    j = 0
    while j + 1 < HEAD_LEVELS and hist[j] > HEAD_CAP:
        j += 1
    head = np.nonzero(lens >= (thr << j))[0]
    return j, head, len(head) > HEAD_CAP          # (clamped: which HEAD_CAP of them survive is a race; no case goes there)


def _window_need(tp, T, t0, end):
    """entries the coarse probe asks for: thread q looks at term t0 + 1 + q * SC_PT"""
    t = t0 + 1 + SC_PT * np.arange(SC_TPB, dtype=np.int64)
    t = t[t <= T]
    s_need = int((tp[t] < end).sum())              # term_ptr is monotone: the threads that see a start inside the chunk are 0 .. s_need-1
    return s_need * SC_PT + SC_PT + 2


def paths(n_docs, term_ptr, post_doc, options):
    """-> (reached: set of path names, detail: dict)."""
    tp = np.asarray(term_ptr, dtype=np.int64)
    pd = np.asarray(post_doc, dtype=np.int64)
    T, P = len(tp) - 1, int(tp[-1])
    lens = np.diff(tp)
    g = geometry(n_docs, P, options)
    reached, d = set(), dict(g)
    # the table's own shape
    if P == 1:
        reached.add("P1")
    reached.add("exact_chunks" if P % SC_CH == 0 else "partial_last_chunk")
    if T and lens[0] == 0:
        reached.add("empty_terms_at_start")
    if T and lens[-1] == 0:
        reached.add("empty_terms_at_end")
    if T and lens[-1] > 0:
        reached.add("last_term_ends_at_last_posting")
    starts = set(tp[:-1][lens > 0].tolist())
    if np.any((lens == SC_CH) & (tp[:-1] % SC_CH == 0)):
        reached.add("term_owns_one_chunk")
    if P > SC_CH and all(b in starts for b in range(SC_CH, P, SC_CH)):
        reached.add("term_boundary_on_every_chunk_boundary")
    if "df_extra" in options:
        reached.add("df_global")
    if not g["bucketed"]:
        reached.add("atomic")
        return reached, d
    reached.add("bucketed")
    shift, nb, per, nblk = g["shift"], g["nb"], g["per"], g["nblk"]
    reached.add(f"shift{shift}")
    if g["shift_forced"]:
        reached.add("shift14_forced")
    reached.add(f"bpt{g['bpt']}")
    if nb > 2048:
        reached.add("nb_gt_2048")
    if nb & 1:
        reached.add("nb_odd")
    if n_docs % (1 << shift) == 0:
        reached.add("n_docs_multiple_of_bucket")
    if n_docs % (1 << shift) == 1 and nb > 1:
        reached.add("last_bucket_one_doc")
    if nblk == 1 and P > SC_CH:
        reached.add("one_block_many_chunks")
    if nblk > 1 and per == SC_CH:
        reached.add("per_8192")
    if nblk > 1 and per > SC_CH:
        reached.add("several_blocks_of_several_chunks")

    # head lists
    thr = g["head_thr"]
    j, head, clamped = head_selection(lens, thr)
    d.update(head_level=j, head_terms=head.tolist(), head_clamped=clamped)
    assert not clamped, "more than HEAD_CAP lists at the last level: the selection is a race, no case may go there"
    hs, he = tp[head], tp[head + 1]
    nh = len(head)
    if thr and int((lens >= thr).sum()) > HEAD_CAP:
        reached.add("more_than_head_cap_qualify")
    if thr:
        reached.add(f"head_level{j}")
    reached.add("head_some" if nh else "head_none")
    if nh:
        eff = thr << j
        if np.any(lens[head] == eff):
            reached.add("head_at_threshold")
        if np.any(lens == eff - 1):
            reached.add("tail_below_threshold")
        if np.any((hs % SC_CH == 0) & (hs > 0)):
            reached.add("head_starts_on_chunk")
        if np.any(he % SC_CH == 0):
            reached.add("head_ends_on_chunk")
        is_head_post = np.zeros(P + 1, dtype=bool)
        for a, b in zip(hs, he):
            is_head_post[a:b] = True
        if np.any((hs % SC_CH != 0) & ~is_head_post[np.maximum(hs - 1, 0)] & (hs > 0)):
            reached.add("head_starts_mid_chunk_after_tail")
        if hs[0] == 0:
            reached.add("head_first_in_table")
        if he[-1] == P:
            reached.add("head_last_in_table")
        # bounds[b][i] (k_head_bounds) -> run lengths [nb][nh]
        runs = np.zeros((nb, nh), dtype=np.int64)
        edges = np.arange(nb + 1, dtype=np.int64) << shift
        for i in range(nh):
            runs[:, i] = np.diff(np.searchsorted(pd[hs[i]:he[i]], edges, side="left"))
        assert (runs.sum(axis=0) == he - hs).all()
        d["head_runs_empty"] = int((runs == 0).sum())
        if d["head_runs_empty"]:
            reached.add("head_run_empty")
        n_live = (runs > 0).sum(axis=0)
        if np.any(n_live == 1):
            reached.add("head_one_bucket")
        if np.any((n_live == 2) & (runs == 1).any(axis=0)):
            reached.add("head_two_buckets_one_single")
        # k_bucket_sum lays a bucket's runs end to end and cuts them into pieces of HEAD_PIECE postings
        pre = np.concatenate([np.zeros((nb, 1), np.int64), np.cumsum(runs, axis=1)], axis=1)
        lo, hi = pre[:, :-1], pre[:, 1:]
        if np.any((hi - 1) // HEAD_PIECE > lo // HEAD_PIECE):
            reached.add("head_piece_crossing")                  # a run continues in the next piece (another wave, or a later turn)
        if np.any((runs > 0) & (lo % HEAD_PIECE != 0)):                      # (lo > 0: earlier runs of the bucket end in this piece)
            reached.add("head_piece_holds_several_runs")
        r0s = np.arange(nblk, dtype=np.int64) * per
        r1s = np.minimum(P, r0s + per)
        for a, b in zip(hs, he):
            if np.any((r0s > a) & (r0s < b)):
                reached.add("block_starts_in_head")
            if np.any((r0s >= a) & (r1s <= b)):
                reached.add("block_inside_head")

    # the chunks of k_scatter<true>, block by block
    chunks = []
    n_global = 0
    for blk in range(nblk):
        r0, r1 = blk * per, min(P, blk * per + per)
        s_t0 = min(int(np.searchsorted(tp[:T], r0, side="right")) - 1, T - 1)      # largest t < T with term_ptr[t] <= r0
        pf = None                                                                  # (pf_t0, pf_need) of the chunk that comes next
        prev_full = None
        for base in range(r0, r1, SC_CH):
            end = min(r1, base + SC_CH)
            n_here = end - base
            over = [i for i in range(nh) if hs[i] < end and he[i] > base]
            assert len(over) <= 2
            rec = {"block": blk, "base": base, "first": base == r0}
            if over and hs[over[0]] <= base and he[over[0]] >= end:
                rec["kind"] = "head_only"
                s_t0, pf, prev_full = int(head[over[0]]), None, None
                chunks.append(rec)
                continue
            rec["kind"] = "all_tail" if not over else ("two_heads" if len(over) == 2 else "mixed")
            live = np.ones(n_here, dtype=bool)
            for i in over:
                live[max(hs[i], base) - base:max(min(he[i], end) - base, 0)] = False
            if pf is not None:
                t0, W, rec["staged"] = pf[0], pf[1], "prefetch"
            else:
                t0, W, rec["staged"] = s_t0, _window_need(tp, T, s_t0, end), "slow"
            assert tp[t0] <= base or not live[0] or t0 == 0, "the window must start at or before the chunk's first posting"
            need = min(SC_WIN, W)
            rec.update(t0=t0, window=W)
            # postings behind the staged window: entry need-1 starts at or before them
            g_here = 0
            if t0 + need - 1 <= T:
                first_behind = max(int(tp[t0 + need - 1]), base)
                if first_behind < end:
                    g_here = int(live[first_behind - base:].sum())
            rec["global"] = g_here
            n_global += g_here
            # where the next chunk's window starts: the term of the last posting the chunk's last thread weighted
            x0 = ((n_here - 1) // SC_PT) * SC_PT
            mine = np.nonzero(live[x0:x0 + SC_PT])[0]
            if len(mine):
                s_t0 = int(np.searchsorted(tp, base + x0 + int(mine[-1]), side="right")) - 1
            else:
                s_t0 = min(int(np.searchsorted(tp, base + x0, side="right")) - 1, t0 + need - 1)
            nbase = base + SC_CH
            pf = None
            if nbase < r1:
                nend = min(r1, nbase + SC_CH)
                n_over = [i for i in range(nh) if hs[i] <= nbase and he[i] >= nend]
                if not n_over:
                    Wn = _window_need(tp, T, s_t0, nend)
                    if Wn <= SC_PF:
                        pf = (s_t0, Wn)
            # the packed 16-bit counters of the chunk
            cnt = np.bincount(pd[base:end][live] >> shift, minlength=nb + 1)
            if prev_full is not None and cnt[prev_full ^ 1] > 0:
                reached.add("hist_full_then_sibling")
            full = np.nonzero(cnt == SC_CH)[0]
            prev_full = int(full[0]) if len(full) else None
            chunks.append(rec)
    d["chunks"] = chunks
    d["n_global_search"] = n_global
    for c in chunks:
        reached.add("chunk_" + c["kind"])
        if c["kind"] == "head_only":
            if c["first"]:
                reached.add("head_only_first_chunk_of_block")
            continue
        reached.add("win_" + c["staged"])
        if c["window"] > SC_PF:
            reached.add("win_gt1024_first_chunk" if c["first"] else "win_gt1024_later_chunk")
        if c["window"] > SC_WIN:
            reached.add("win_gt_sc_win")
        if c["global"]:
            reached.add("win_global_search")
            if not c["first"]:
                reached.add("win_global_search_later_chunk")
    # k_weight_count walks the same ranges in chunks of CH and skips the ones a head list covers
    for a, b in zip(hs, he):
        if _div_up(int(a), CH) * CH + CH <= int(b):
            reached.add("count_chunk_head_only")
    return reached, d


# every path this suite claims; test_tfidf_cases_cpu.py demands a case for each
REQUIRED_PATHS = (
    "atomic", "bucketed", "shift10", "shift13", "shift14", "shift14_forced", "bpt2", "bpt4", "nb_gt_2048", "nb_odd",
    "n_docs_multiple_of_bucket", "last_bucket_one_doc", "one_block_many_chunks", "per_8192", "several_blocks_of_several_chunks",
    "block_starts_in_head", "block_inside_head",
    "P1", "partial_last_chunk", "exact_chunks", "empty_terms_at_start", "empty_terms_at_end", "last_term_ends_at_last_posting",
    "term_owns_one_chunk", "term_boundary_on_every_chunk_boundary",
    "head_none", "head_some", "head_level0", "head_level1", "more_than_head_cap_qualify", "head_at_threshold", "tail_below_threshold",
    "head_starts_on_chunk", "head_ends_on_chunk", "head_starts_mid_chunk_after_tail", "head_first_in_table", "head_last_in_table",
    "head_run_empty", "head_two_buckets_one_single", "head_piece_crossing", "head_piece_holds_several_runs",
    "chunk_all_tail", "chunk_mixed", "chunk_head_only", "chunk_two_heads", "head_only_first_chunk_of_block", "count_chunk_head_only",
    "win_slow", "win_prefetch", "win_gt1024_first_chunk", "win_gt1024_later_chunk", "win_gt_sc_win", "win_global_search",
    "win_global_search_later_chunk", "hist_full_then_sibling", "df_global",
)
# "head_one_bucket" (a head list with all its postings in one bucket) cannot exist: a head list holds at least 2 * SC_CH + 1 = 16385
# postings of distinct docs and the largest bucket holds 2^14 = 16384 docs.  "head_two_buckets_one_single" is the nearest table.
IMPOSSIBLE_PATHS = ("head_one_bucket",)

EDGE_KINDS = ("tf_zero", "tf_denormal", "sq_denormal", "sq_underflow", "sq_overflow", "idf_zero", "idf_negative", "idf_neginf", "w_nan")
REQUIRED_VALUE_PATHS = tuple(f"{k}@{where}" for k in EDGE_KINDS for where in ("head", "tail"))


def value_paths(case, w, idf, head_terms):
    """Float32 edges in the ORACLE's results (w, idf) of a case, told apart by where the posting sits (head or tail list)."""
    tp = np.asarray(case.term_ptr, dtype=np.int64)
    tf = np.asarray(case.tf, dtype=np.float32)
    lens = np.diff(tp)
    term_of = np.repeat(np.arange(len(lens)), lens)
    in_head = np.isin(term_of, np.asarray(head_terms, dtype=np.int64))
    tiny = np.finfo(np.float32).tiny
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        sq = (w * w).astype(np.float32)
    f = idf[term_of]
    kinds = {
        "tf_zero": tf == 0, "tf_denormal": (tf != 0) & (np.abs(tf) < tiny),
        "sq_denormal": (sq > 0) & (sq < tiny), "sq_underflow": (w != 0) & (sq == 0), "sq_overflow": np.isfinite(w) & np.isinf(sq),
        "idf_zero": f == 0, "idf_negative": (f < 0) & np.isfinite(f), "idf_neginf": np.isneginf(f), "w_nan": np.isnan(w),
    }
    out = set()
    for k, m in kinds.items():
        if np.any(m & in_head):
            out.add(k + "@head")
        if np.any(m & ~in_head):
            out.add(k + "@tail")
    # every such posting sits in a doc of its own: the order of the sum cannot matter
    edge = np.zeros(len(tf), dtype=bool)
    for m in kinds.values():
        edge |= m
    per_doc = np.bincount(np.asarray(case.post_doc, dtype=np.int64), minlength=case.n_docs)
    assert (per_doc[np.asarray(case.post_doc, dtype=np.int64)[edge]] == 1).all(), "an edge value shares its doc"
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# what the oracle says

def whole_table(case):
    """A shard case as the whole corpus the oracle can weight: term t's local postings, then df_extra[t] postings of docs beyond
    the shard.  -> (n_docs_whole, term_ptr, post_doc, local: bool per posting)."""
    tp = np.asarray(case.term_ptr, dtype=np.int64)
    extra = np.asarray(case.options["df_extra"], dtype=np.int64)
    lens = np.diff(tp)
    wl = lens + extra
    wtp = np.concatenate([[0], np.cumsum(wl)]).astype(np.uint64)
    term_of = np.repeat(np.arange(len(wl)), wl)
    k = np.arange(int(wl.sum()), dtype=np.int64) - np.asarray(wtp, dtype=np.int64)[term_of]      # position inside the term
    local = k < lens[term_of]
    docs = np.where(local, 0, case.n_docs + k - lens[term_of])
    docs[local] = np.asarray(case.post_doc, dtype=np.int64)
    return case.n_docs + int(extra.max(initial=0)), wtp, docs.astype(np.uint32), local


def expected(case, tfidf):
    """The first and the second ss_tfidf_build of the case, by `tfidf` (oracle.tfidf or a stand-in with its signature):
    -> idf float32[T], (w1, mag1), (w2, mag2).  The second build multiplies the stored weights again (term_weighting.go:42)."""
    if "df_extra" not in case.options:
        w1, m1, idf = tfidf(case.term_ptr, case.post_doc, case.tf, case.total_docs, case.n_docs)
        w2, m2, _ = tfidf(case.term_ptr, case.post_doc, w1, case.total_docs, case.n_docs)
        return idf, (w1, m1), (w2, m2)
    n_whole, wtp, wdocs, local = whole_table(case)
    tf = np.ones(len(wdocs), dtype=np.float32)
    tf[local] = case.tf
    w1, m1, idf = tfidf(wtp, wdocs, tf, case.total_docs, n_whole)
    w2, m2, _ = tfidf(wtp, wdocs, w1, case.total_docs, n_whole)
    return idf, (w1[local], m1[:case.n_docs]), (w2[local], m2[:case.n_docs])


def exactness(n_docs, post_doc, w, use_fraction=False):
    """Are the float64 sums of the float32 squares of `w` exact in ANY order?  Per doc: every square is an integer multiple of
    2^e (e = the lowest set bit among the doc's squares) and the integers sum to less than 2^53, so every partial sum of every order
    is a float64.  -> (ok bool[n_docs], nonfinite bool[n_docs], exact float64[n_docs]); docs that hold an inf or NaN square are
    reported apart (no rational value).  use_fraction: the same through fractions.Fraction, posting by posting (small tables)."""
    pd = np.asarray(post_doc, dtype=np.int64)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        sq = (np.asarray(w, dtype=np.float32) * np.asarray(w, dtype=np.float32)).astype(np.float32).astype(np.float64)
    fin = np.isfinite(sq)
    nonfinite = np.bincount(pd[~fin], minlength=n_docs) > 0
    if use_fraction:
        tot = [Fraction(0)] * n_docs
        f64 = np.zeros(n_docs)
        for d_, s_ in zip(pd[fin].tolist(), sq[fin].tolist()):
            tot[d_] += Fraction(s_)
            f64[d_] += s_                                                   # posting order, as the oracle sums
        ok = np.array([Fraction(float(a)) == b for a, b in zip(f64.tolist(), tot)])
        return ok | nonfinite, nonfinite, f64
    nz = fin & (sq != 0)
    m, e = np.frexp(sq[nz])
    mi = np.ldexp(m, 24).astype(np.int64)                                   # a float32 has 24 significant bits
    assert (np.ldexp(mi.astype(np.float64), e - 24) == sq[nz]).all()
    e = e.astype(np.int64) - 24
    docs = pd[nz]
    emin = np.full(n_docs, np.iinfo(np.int64).max)
    np.minimum.at(emin, docs, e)
    sh = e - emin[docs]
    ok = np.ones(n_docs, dtype=bool)
    wide = sh > 28                                                          # 24 + 28 + (bits of the count) must stay below 63
    ok[docs[wide]] = False
    tot = np.zeros(n_docs, dtype=np.int64)
    np.add.at(tot, docs[~wide], mi[~wide] << sh[~wide])
    cnt = np.bincount(docs, minlength=n_docs)
    ok &= cnt < (1 << 10)
    ok &= tot < (1 << 53)
    exact = np.where(cnt > 0, np.ldexp(tot.astype(np.float64), np.where(cnt > 0, emin, 0).astype(np.int64)), 0.0)
    return ok | nonfinite, nonfinite, exact


# ---------------------------------------------------------------------------------------------------------------------------------
# builders

def make_tf(n):
    """0.5 .. 1.0 in eighths: short mantissas, so that the squares of a doc sum exactly"""
    return ((4 + (np.arange(n, dtype=np.int64) * 7) % 5) / 8.0).astype(np.float32)


def spread(length, n_docs, phase=0, lo=0):
    """`length` strictly ascending doc ids spread evenly over [lo, n_docs)"""
    span = n_docs - lo
    assert 0 < length <= span
    return lo + (np.arange(length, dtype=np.int64) * span + (phase % span)) // length


def run_of(length, first):
    return first + np.arange(length, dtype=np.int64)


class _Table:
    def __init__(self, n_docs):
        self.n_docs, self.lists, self.n_post = n_docs, [], 0

    def add(self, docs):
        docs = np.asarray(docs, dtype=np.int64)
        assert len(docs) == 0 or (np.all(np.diff(docs) > 0) and docs[0] >= 0 and docs[-1] < self.n_docs)
        self.lists.append(docs)
        self.n_post += len(docs)
        return len(self.lists) - 1

    def empty(self, n=1):
        for _ in range(n):
            self.add(np.zeros(0, np.int64))

    def small_until(self, target, max_len=37, mul=5):
        """short tail lists (1 .. max_len postings) until the table holds exactly `target` postings"""
        k = len(self.lists)
        while self.n_post < target:
            ln = min((k * mul) % max_len + 1, target - self.n_post)
            stride = 1 + k % 3
            first = (k * 131) % (self.n_docs - ln * stride)
            self.add(first + np.arange(ln, dtype=np.int64) * stride)
            k += 1

    def finish(self):
        tp = np.concatenate([[0], np.cumsum([len(x) for x in self.lists])]).astype(np.uint64)
        pd = (np.concatenate(self.lists) if self.n_post else np.zeros(0, np.int64)).astype(np.uint32)
        return tp, pd


def _case(name, tab, total_docs, options, expect, tf=None):
    tp, pd = tab.finish()
    return Case(name, tab.n_docs, tp, pd, make_tf(len(pd)) if tf is None else tf, total_docs, dict(options), frozenset(expect))


TAIL_OPTS = {"tfidf.bucket_min": 1, "tfidf.head_min_run": 0}
HEAD_OPTS = {"tfidf.bucket_min": 1, "tfidf.head_min_run": 1}


def _ends(n_post, tight=False):
    """A: table ends and chunk edges — n_post postings in short lists; empty terms at both ends unless tight"""
    def build():
        tab = _Table(2500)
        if not tight:
            tab.empty(3)
        tab.small_until(n_post)
        if not tight:
            tab.empty(2)
        exp = {"bucketed", "shift10", "bpt2", "nb_odd", "head_none", "chunk_all_tail", "win_slow",
               "exact_chunks" if n_post % SC_CH == 0 else "partial_last_chunk"}
        exp |= {"last_term_ends_at_last_posting"} if tight else {"empty_terms_at_start", "empty_terms_at_end"}
        if n_post == 1:
            exp.add("P1")
        if n_post > SC_CH:
            exp.add("per_8192")
        return _case(f"A.P{n_post}" + (".tight" if tight else ""), tab, 4096, {**TAIL_OPTS, "tfidf.bucket_shift": 10}, exp)
    return build


def _own_chunk():
    tab = _Table(9000)
    for k in range(3):
        tab.add(spread(SC_CH, 9000, phase=k * 1000))
        tab.empty(k)                                                        # empty terms that start ON the chunk boundary
    tab.small_until(3 * SC_CH + 700)
    return _case("A.own_chunk", tab, 16384, {**TAIL_OPTS, "tfidf.bucket_shift": 10},
                 {"term_owns_one_chunk", "term_boundary_on_every_chunk_boundary", "per_8192", "win_slow"})


def _window_table():
    """W: ~20k terms, 6 chunks.  Chunks 0 and 3 hold a run of 8300 empty terms between two non-empty terms; chunks 1, 2 and 4 span more
    than 1024 non-empty terms (lists of 1 to 7 postings); chunk 5 holds ordinary lists (a window the prefetch takes)."""
    tab = _Table(20000)
    tab.small_until(300)
    tab.empty(8300)
    tab.small_until(SC_CH + 100)                                            # chunk 0
    tab.small_until(3 * SC_CH + 500, max_len=7, mul=3)                      # chunks 1, 2: ~2000 terms each
    tab.empty(8300)                                                         # ... behind the first 500 postings of chunk 3
    tab.small_until(4 * SC_CH - 50)
    tab.small_until(5 * SC_CH - 20, max_len=7, mul=3)                       # chunk 4
    tab.small_until(6 * SC_CH - 1000, max_len=37)                           # chunk 5
    tab.add(spread(900, 20000, phase=77))
    return tab


def _window(blocks):
    def build():
        opts = dict(TAIL_OPTS)
        exp = {"win_slow", "win_gt1024_first_chunk", "win_gt_sc_win", "win_global_search"}
        if blocks is not None:
            opts["tfidf.blocks"] = blocks
        if blocks == 1:
            exp |= {"one_block_many_chunks", "win_gt1024_later_chunk", "win_global_search_later_chunk", "win_prefetch"}
        if blocks == 3:
            exp |= {"several_blocks_of_several_chunks", "win_gt1024_later_chunk"}
        return _case("W.windows" + ("" if blocks is None else f".b{blocks}"), _window_table(), 20000, opts, exp)
    return build


def _head_table():
    """H: six head lists (L >= 16385 with tfidf.head_min_run = 1 and 5 buckets) placed against the chunk grid; see the expectations"""
    n = 40000
    tab = _Table(n)
    h = [tab.add(spread(16385, n))]                                         # first in the table, exactly at the threshold
    tab.add(spread(16384, n, phase=11))                                     # one short: a tail list
    tab.small_until(36000)                                                  # 36000 = chunk 4 + 3232
    h.append(tab.add(spread(7 * SC_CH - 36000, 32768, lo=8192)))            # starts mid-chunk behind tails, ends ON a boundary; no docs in buckets 0 and 4
    h.append(tab.add(spread(19385, n, phase=5)))                            # starts ON a boundary, ends mid-chunk ...
    h.append(tab.add(run_of(20000, 0)))                                     # ... where the next begins; consecutive docs: runs of 8192, 8192, 3616
    tab.small_until(100000)
    h.append(tab.add(spread(16385, n, phase=23)))                           # last in the table
    return tab, h


HEAD_EXPECT = {"head_some", "head_level0", "head_at_threshold", "tail_below_threshold", "head_starts_on_chunk", "head_ends_on_chunk",
               "head_starts_mid_chunk_after_tail", "head_first_in_table", "head_last_in_table", "head_run_empty", "head_piece_crossing",
               "head_piece_holds_several_runs", "chunk_all_tail", "chunk_mixed", "chunk_head_only", "chunk_two_heads", "nb_odd", "shift13",
               "count_chunk_head_only", "last_term_ends_at_last_posting"}


def _heads(blocks, shard=False):
    def build():
        tab, h = _head_table()
        opts = dict(HEAD_OPTS)
        exp = set(HEAD_EXPECT)
        if blocks is not None:
            opts["tfidf.blocks"] = blocks
        if blocks == 1:
            exp |= {"one_block_many_chunks", "win_prefetch"}
        elif blocks == 3:
            exp |= {"several_blocks_of_several_chunks", "block_starts_in_head", "head_only_first_chunk_of_block", "win_prefetch"}
        else:
            exp |= {"per_8192", "block_starts_in_head", "block_inside_head", "head_only_first_chunk_of_block"}
        total = 40000
        if shard:
            opts["df_extra"] = (np.arange(len(tab.lists), dtype=np.int64) * 3) % 11
            exp.add("df_global")
            total = 40011
        name = "H.heads" + ("" if blocks is None else f".b{blocks}") + (".shard" if shard else "")
        return _case(name, tab, total, opts, exp)
    return build


def _many_heads():
    """M: 1000 lists of 16385 .. 16400 postings and 100 of 32770 .. 32788 over 40000 docs: 1100 lists reach the threshold, more than
    HEAD_CAP, so the threshold doubles once and exactly the 100 long lists stay head"""
    n = 40000
    tab = _Table(n)
    for k in range(1100):
        if k % 11 == 5:
            tab.add(spread(32770 + (k % 7) * 3, n, phase=k * 977))
        else:
            tab.add(spread(16385 + k % 16, n, phase=k * 977))
    return _case("M.many_heads", tab, 40000, {**HEAD_OPTS, "tfidf.blocks": 256},
                 {"more_than_head_cap_qualify", "head_level1", "head_some", "several_blocks_of_several_chunks", "chunk_head_only",
                  "chunk_mixed", "chunk_all_tail", "win_prefetch", "block_starts_in_head"})


def _bpt4():
    n = 2_200_000
    tab = _Table(n)
    tab.add(spread(140000, n, phase=3))                                     # >= 64 * 2149 postings: head at the default run length
    for k in range(75):
        tab.add(spread(2000, n, phase=k * 29989 + 7))
    return _case("G.bpt4", tab, 1 << 22, {"tfidf.bucket_min": 1, "tfidf.head_min_run": 64, "tfidf.bucket_shift": 10},
                 {"shift10", "bpt4", "nb_gt_2048", "nb_odd", "head_some", "per_8192"})


def _multiple(extra):
    def build():
        n = 3 * 1024 + extra
        tab = _Table(n)
        for k in range(12):
            tab.add(spread(1500 + k, n, phase=k * 401))
        tab.add(run_of(200, n - 200))                                       # the last docs, the very last one among them
        tab.small_until(20000)
        exp = {"shift10", "last_bucket_one_doc"} if extra else {"shift10", "n_docs_multiple_of_bucket", "nb_odd"}
        return _case("G.plus1" if extra else "G.exact", tab, 4096, {**TAIL_OPTS, "tfidf.bucket_shift": 10}, exp)
    return build


def _full_bucket():
    """a chunk whose 8192 postings all fall into one bucket (its 16-bit counter reads 8192), the sibling bucket of the same word
    in the next chunk — in both orders"""
    n = 16384
    tab = _Table(n)
    for first in (0, 8192, 8192, 0):
        tab.add(run_of(8192, first))
    tab.small_until(4 * SC_CH + 5000)
    return _case("G.full_bucket", tab, 16384, {**TAIL_OPTS, "tfidf.blocks": 1},
                 {"hist_full_then_sibling", "one_block_many_chunks", "shift13", "n_docs_multiple_of_bucket", "term_owns_one_chunk"})


def _shift14():
    n = 40000
    tab = _Table(n)
    tab.small_until(3000)
    tab.add(run_of(16385, 16383))                                           # one doc of bucket 0, all 16384 of bucket 1, none of bucket 2
    for k in range(8):
        tab.add(spread(2500, n, phase=k * 1777))
    return _case("G.shift14", tab, 40000, {**HEAD_OPTS, "tfidf.bucket_shift": 14},
                 {"shift14", "nb_odd", "head_some", "head_two_buckets_one_single", "head_run_empty", "head_piece_crossing"})


def _forced14():
    n = (1 << 22) + 5
    tab = _Table(n)
    for k in range(30):
        tab.add(spread(3000, n, phase=k * 139999))
    tab.add(run_of(40, n - 40))
    return _case("G.forced14", tab, 1 << 23, {"tfidf.bucket_min": 1, "tfidf.head_min_run": 64, "tfidf.bucket_shift": 10},
                 {"shift14", "shift14_forced", "nb_odd", "head_none"})


EDGE_TF = np.array([0.0, -0.0, 1e-45, 1e-40, -1e-40, 1.17549435e-38, 1e-20, 3e-20, 1e-25, -1e-25, 1e20, -1e20, 3e38, 2.5e19],
                   dtype=np.float32)


def _edges(total_docs):
    """F: one head list (docs 0 .. 16999) and one tail list (docs 20000 .. 29999) that share no doc, so every doc holds ONE posting
    and no sum has an order.  The edge values sit in head-only chunks, in the mixed chunk and in the tail list."""
    def build():
        tab = _Table(40000)
        tab.add(run_of(17000, 0))
        tab.add(run_of(10000, 20000))
        tp, pd = tab.finish()
        tf = make_tf(len(pd))
        k = len(EDGE_TF)
        tf[100:100 + 13 * k:13] = EDGE_TF                                   # head list, head-only chunk
        tf[16500:16500 + k] = EDGE_TF                                       # head list, the chunk it shares with the tail list
        tf[17000 + 50:17000 + 50 + 11 * k:11] = EDGE_TF                     # tail list, same chunk
        tf[26000:26000 + k] = EDGE_TF                                       # tail list, last chunk
        return Case(f"F.total{total_docs}", 40000, tp, pd, tf, total_docs, dict(HEAD_OPTS),
                    frozenset({"head_some", "chunk_head_only", "chunk_mixed", "chunk_all_tail", "head_first_in_table"}))
    return build


def _atomic():
    tab = _Table(5000)
    tab.empty(2)
    tab.small_until(CH + 77)
    tab.empty(1)
    return _case("A.atomic", tab, 5000, {}, {"atomic", "empty_terms_at_start", "empty_terms_at_end"})


_BUILDERS = {}
for _b, _n in [(_atomic, "A.atomic")] + \
        [(_ends(p), f"A.P{p}") for p in (1, 8191, 8192, 8193, 3 * 8192)] + [(_ends(8193, True), "A.P8193.tight"), (_own_chunk, "A.own_chunk")] + \
        [(_window(b), "W.windows" + ("" if b is None else f".b{b}")) for b in (None, 1, 3)] + \
        [(_heads(b), "H.heads" + ("" if b is None else f".b{b}")) for b in (None, 1, 3, 1 << 20)] + \
        [(_heads(b, True), "H.heads" + ("" if b is None else f".b{b}") + ".shard") for b in (None, 1)] + \
        [(_many_heads, "M.many_heads"), (_bpt4, "G.bpt4"), (_multiple(0), "G.exact"), (_multiple(1), "G.plus1"),
         (_full_bucket, "G.full_bucket"), (_shift14, "G.shift14"), (_forced14, "G.forced14")] + \
        [(_edges(t), f"F.total{t}") for t in (40000, 17000, 10000, 5000, 0)]:
    _BUILDERS[_n] = _b
CASE_NAMES = tuple(_BUILDERS)
# cases with docs whose square is inf or NaN (no rational sum): compared bit for bit all the same — every such doc holds one posting
NONFINITE_CASES = tuple(n for n in CASE_NAMES if n.startswith("F."))


@functools.lru_cache(maxsize=None)
def get_case(name):
    c = _BUILDERS[name]()
    assert c.name == name, (c.name, name)
    for a in (c.term_ptr, c.post_doc, c.tf):
        a.setflags(write=False)
    return c
