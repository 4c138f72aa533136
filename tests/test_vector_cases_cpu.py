"""CPU side of the vector path suite (tests/vector_cases.py): what a reviewer can check without a GPU.

  * Every case reaches the path it is named for: the replay of the kernels' list bookkeeping, run with the product planner's cap,
    query block, chunk size and `tight`, reports the in-loop cuts, `n` and the holes at each cut and the thresholds, and the counts
    are asserted here.
  * The replay itself is checked: its last lists, merged, are the rows of tests/vector_model.py / tests/vector_lists_model.py.
  * The control: test_gpu_vector.py's largest 64-dim shape under the default plan makes no in-loop cut at all, which is why
    tests/test_gpu_vector_paths.py exists.
"""
import numpy as np
import pytest

from tests import vector_cases as vc

_SEEN = {}           # case name -> facts of its replay; read by test_every_path_is_reached


def facts(name):
    if name in _SEEN:
        return _SEEN[name]
    case = vc.get_case(name)
    reps = vc.replay_case(case)
    p, k = case.plan, case.k
    cuts = [c for r in reps.values() for c in r.cuts]
    f = dict(case=case, reps=reps, plan=p, cuts=cuts,
             holes={c["holes"] for c in cuts if c["holes"][0] == c["holes"][1]},
             late_steps={c["step"] for c in cuts if c["step"] != 0},
             n_at_cut={c["n"] for c in cuts})
    # a block (an item's group of queries) in which, at one check, some lists are cut and some are not
    f["split_checks"] = 0
    if case.kind == "exact":
        for c in range(p["n_chunks"]):
            for b in range(p["n_qblocks"]):
                qs = range(b * p["q_block"], min((b + 1) * p["q_block"], len(case.qvec)))
                for i in range(len(reps[c, qs[0]].checks)):
                    cut = {reps[c, q].checks[i][3] for q in qs}
                    f["split_checks"] += cut == {True, False}
    elif len(case.qvec) <= p["q_block"] and case.n_probe == 1:              # (one group: every query shares the item)
        n_checks = len(reps[0, 0, 0].checks)
        for i in range(n_checks):
            f["split_checks"] += {r.checks[i][3] for r in reps.values()} == {True, False}
    print(f"{name}: q_block={p['q_block']} cap={p['cap']} tight={p['tight']} lists={len(reps)} cuts={len(cuts)} "
          f"n_at_cut={sorted(f['n_at_cut'])[:6]} holes={sorted(f['holes'])[:6]} late_steps={sorted(f['late_steps'])} split={f['split_checks']}")
    _SEEN[name] = f
    return f


@pytest.mark.parametrize("name", vc.CASE_NAMES + [vc.CONTROL])
def test_replay_gives_the_model_rows(name):
    f = facts(name)
    got, want = vc.merged_rows(f["case"], f["reps"]), vc.model_rows(f["case"])
    assert got[1].tolist() == want[1].tolist()
    assert got[0].tobytes() == want[0].tobytes()
    for r in f["reps"].values():                                             # the bookkeeping's own claims
        assert len(r.final) <= f["case"].k and all(n <= f["plan"]["cap"] for _, _, n, _ in r.checks)
        assert all(c["n"] > f["case"].k and c["n"] + f["plan"]["inc"] > f["plan"]["cap"] for c in r.cuts)


def test_control_default_plan_never_cuts_in_the_loop():
    f = facts(vc.CONTROL)
    p = f["plan"]
    assert (p["chunk_docs"], p["n_chunks"]) == (vc.ROUND, 17)                 # one round per chunk
    assert len(f["cuts"]) == 0
    assert all(len(r.checks) == 1 and r.checks[0][2] == 0 for r in f["reps"].values())   # no check ever sees a key
    for (c, q), r in f["reps"].items():                                       # only the cut behind the loop runs, with n <= 256
        assert (r.end_cut is None) == (c == 16) and (c == 16 or r.end_cut["n"] == vc.ROUND) and len(r.final) == (3 if c == 16 else 10)
    assert {c["thr"] for r in f["reps"].values() for c in r.cuts} == set()    # every compare against threshold 0


def test_plans_are_what_the_cases_assume():
    plan = lambda n: vc.get_case(n).plan                                      # noqa: E731
    for name in ("rising", "falling", "exact_fill", "mixed_block", "masked_winners", "lists_rising", "lists_falling", "lists_mixed_block"):
        assert (plan(name)["q_block"], plan(name)["tight"]) == (32, False), name
    assert plan("rising")["cap"] == plan("exact_fill")["cap"] == 292          # (17 queries: a block of 32; a block of 16 would have 424)
    assert (plan("plateau")["q_block"], plan("plateau")["cap"], plan("plateau")["tight"]) == (16, 424, False)
    for name in ("tight_k100", "lists_tight_k100"):
        assert (plan(name)["q_block"], plan(name)["cap"], plan(name)["tight"]) == (32, 292, True), name
    assert plan("tight_k100")["n_qblocks"] == 2
    assert (plan("tight_k1024")["q_block"], plan("tight_k1024")["cap"], plan("tight_k1024")["tight"]) == (16, 1240, True)
    for n_q, blocks in ((64, 1), (65, 2), (130, 3)):
        p = plan(f"query_blocks_{n_q}")
        assert (p["q_block"], p["n_qblocks"], p["tight"]) == (64, blocks, True) and p["cap"] >= 10 + vc.TILE
    assert [plan(f"random_k{k}")["tight"] for k in (1, 10, 100, 1024)] == [False, False, False, True]
    for name in vc.CASE_NAMES:
        case, p = vc.get_case(name), plan(name)
        if case.kind == "exact":
            assert p["n_chunks"] == (2 if "two_chunks" in name or name == "masked_winners" else 1), name
        else:
            assert p["seg_rows"] == case.options["vec.list_seg_rows"] and len(vc.list_rows(case.lod, 0)) == 2304 >= 2048


def later(rep):
    return rep.cuts[1:]


def test_rising():
    for name in ("rising", "lists_rising"):
        f = facts(name)
        k = f["case"].k
        for r in f["reps"].values():
            assert [c[3] for c in r.checks] == [False] + [True] * (len(r.checks) - 1)     # every check after round 0 cuts
            assert len(r.cuts) == (15 if name == "rising" else 8)
            assert all(c["holes"] == (k, k) for c in later(r)) and all(c["n"] == k + vc.ROUND for c in later(r))
            thr = [c["thr"] for c in r.cuts]
            assert thr == sorted(thr) and len(set(thr)) == len(thr)
        assert {r.cuts[0]["n"] for r in f["reps"].values() if r.cuts} == {vc.ROUND}


def test_falling():
    for name in ("falling", "lists_falling"):
        f = facts(name)
        k = f["case"].k
        docs = np.arange(vc.N_DOCS) if name == "falling" else vc.list_rows(f["case"].lod, 0)
        for key, r in f["reps"].items():
            q = key[1] if name == "falling" else key[0]
            assert len(r.cuts) == 1 and r.end_cut is None
            cut = r.cuts[0]
            after = [c for c in r.checks if (c[0], c[1]) > (cut["round"], cut["step"])]
            assert after and all(n == k for _, _, n, _ in after)                            # nothing passes the threshold again
            assert vc.rows_of(r.final)["doc"].tolist() == docs[:k].tolist()
            if q == 16:
                assert (cut["round"], cut["n"], cut["holes"]) == (2, k + vc.ROUND, (0, 0))
            else:
                assert (cut["round"], cut["n"]) == (1, vc.ROUND) and cut["holes"][0] <= cut["holes"][1] <= k


def test_plateau():
    for name in ("plateau", "lists_plateau"):
        f = facts(name)
        k = f["case"].k
        reps = sorted(f["reps"].items())
        flat, steps = reps[0][1], reps[1][1]
        assert len(flat.cuts) == 1 and flat.cuts[0]["n"] == vc.ROUND and flat.end_cut is None
        assert all(n == k for _, _, n, _ in flat.checks[2:])                                # equal scores: the doc id fails `key > thr`
        assert vc.rows_of(flat.final)["doc"].tolist() == (np.arange(k) if name == "plateau" else vc.list_rows(f["case"].lod, 0)[:k]).tolist()
        assert len(set(vc.rows_of(flat.final)["score"].tolist())) == 1
        assert len(steps.cuts) >= 3 and len({c["thr"] >> 32 for c in steps.cuts}) >= 3      # the other query of the block keeps cutting
        assert f["split_checks"] >= 1


def test_exact_fill():
    f = facts("exact_fill")
    p = f["plan"]
    r = f["reps"][0, 0]
    assert r.checks[1] == (1, 0, p["cap"] - vc.ROUND, False) and r.checks[1][2] + p["inc"] == p["cap"]
    assert r.checks[2] == (2, 0, p["cap"], True) and r.cuts[0]["n"] == p["cap"]
    assert p["cap"] in f["n_at_cut"]
    assert f["reps"][0, 1].checks[1] == (1, 0, vc.ROUND, True)                # the plain queries of the block were cut one check before
    assert f["split_checks"] >= 1


def test_mixed_block():
    for name, unmasked in (("mixed_block", range(12)), ("lists_mixed_block", range(17))):
        f = facts(name)
        case, k = f["case"], f["case"].k
        n_q = len(case.qvec)
        assert f["plan"]["q_block"] >= n_q
        rep = (lambda q: f["reps"][0, q]) if name == "mixed_block" else (lambda q: f["reps"][q, 0, 0])
        n_cuts = [len(rep(q).cuts) for q in range(n_q)]
        few, none = (12, 13) if name == "mixed_block" else (17, 18)
        assert max(n_cuts) >= 8 and 1 in n_cuts and n_cuts[few] == n_cuts[none] == 0
        assert len(rep(few).final) == 7 < k and len(rep(none).final) == 0
        assert f["split_checks"] >= 5
        want = vc.model_rows(case)[1]
        assert want[few] == 7 and want[none] == 0 and (want[list(unmasked)] == k).all()


def test_masked_winners():
    f = facts("masked_winners")
    case = f["case"]
    assert case.masks.shape[1] == 2080 and -(-2080 // 32) == 65
    for (c, q), r in f["reps"].items():
        assert len(r.cuts) >= (1 if case.mask_id[q] >= 0 else 3), (c, q)
    rows, n = vc.model_rows(case)
    for q in range(len(case.qvec)):
        end = {1087, 2079} & set(rows["doc"][q, :n[q]].tolist())
        assert bool(end) == (case.mask_id[q] < 0)                             # the masked winners are winners without the mask


def test_tight_cases():
    for name in ("tight_k100", "lists_tight_k100"):
        f = facts(name)
        assert f["plan"]["tight"] and f["late_steps"] == {1, 2, 3}            # cuts inside a round, not only at its first step
        assert f["plan"]["cap"] in f["n_at_cut"]                              # (228 + 64 == cap: a list filled to its last slot)
        assert all(f["plan"]["cap"] - vc.TILE < n <= f["plan"]["cap"] for n in f["n_at_cut"])
        assert {h for h, _ in f["holes"]} - {0, 100}
    f = facts("tight_k1024")
    p = f["plan"]
    assert p["tight"] and f["late_steps"]
    assert all(p["cap"] - vc.TILE < n <= p["cap"] for n in f["n_at_cut"])     # within 64 of cap
    assert (192, 192) in f["holes"] and all(0 < lo < 1024 for lo, _ in f["holes"])
    assert f["reps"][0, 0].cuts[0]["holes"] == (192, 192)                    # 16 whole steps fill the first 1024 slots: no order enters
    for name in ("query_blocks_64", "query_blocks_65", "query_blocks_130"):
        f = facts(name)
        assert f["late_steps"] == {1, 2, 3} and f["split_checks"] >= 10


def test_two_chunks_and_two_segments_both_cut():
    for name in ("rising_two_chunks", "tight_k100_two_chunks", "tight_k1024_two_chunks"):
        f = facts(name)
        assert f["plan"]["n_chunks"] == 2
        for q in range(len(f["case"].qvec)):
            if name == "tight_k100_two_chunks" and q % 3 == 2:
                assert len(f["reps"][0, q].cuts) >= 1                         # (a falling query: nothing of the second chunk passes ...
                continue                                                     # ... threshold 0 is per chunk, so it does cut there too)
            assert len(f["reps"][0, q].cuts) >= 1 and len(f["reps"][1, q].cuts) >= 1, (name, q)
        one = vc.get_case(f["case"].same_rows_as)
        assert one.vec.tobytes() == f["case"].vec.tobytes() and one.qvec.tobytes() == f["case"].qvec.tobytes() and one.k == f["case"].k
    f = facts("lists_two_segments")
    segs = {key[2] for key in f["reps"] if key[1] == 0}
    assert segs == {0, 1}
    for q in range(len(f["case"].qvec)):
        assert len(f["reps"][q, 0, 0].cuts) >= 3 and len(f["reps"][q, 0, 1].cuts) >= 3


def test_random_cases_move_a_threshold():
    for k in (1, 10, 100, 1024):
        f = facts(f"random_k{k}")
        for r in f["reps"].values():
            assert len(r.cuts) >= (2 if k >= 100 else 1)
            thr = [c["thr"] for c in r.cuts] + ([r.end_cut["thr"]] if r.end_cut else [])
            assert thr == sorted(thr) and len(set(thr)) == len(thr)
            behind = r.appended - r.cuts[0]["appended_since"]                 # docs that passed a threshold above 0: some, not all
            assert 0 < behind < vc.N_DOCS // 2
        if k >= 100:
            assert any(0 < lo == hi < k for lo, hi in f["holes"])             # only some of the kept keys fall out


def test_every_path_is_reached():
    names = vc.CASE_NAMES
    claims_cuts = [n for n in names]                                          # every case the device runs claims an in-loop cut
    for n in claims_cuts:
        assert len(facts(n)["cuts"]) >= 1, n
        for r in facts(n)["reps"].values():
            assert all(c["thr"] > 0 for c in r.cuts)
    holes = set().union(*(facts(n)["holes"] for n in names))
    ks = {n: facts(n)["case"].k for n in names}
    assert any((ks[n], ks[n]) in facts(n)["holes"] for n in names)            # holes == k
    assert any((0, 0) in facts(n)["holes"] for n in names)                    # holes == 0
    assert any(0 < lo < ks[n] for n in names for lo, _ in facts(n)["holes"])  # 0 < holes < k
    assert holes
    for kind in ("exact", "lists"):
        of = [n for n in names if facts(n)["case"].kind == kind]
        assert any(facts(n)["late_steps"] for n in of), kind
        assert any(facts(n)["split_checks"] for n in of), kind
        assert any(facts(n)["plan"]["cap"] in facts(n)["n_at_cut"] for n in of), kind
    assert {facts(n)["plan"]["q_block"] for n in names if facts(n)["case"].kind == "exact"} == {16, 32, 64}
    assert max(facts(n)["plan"]["n_qblocks"] for n in names if facts(n)["case"].kind == "exact") == 3


def test_list_rows_are_the_stable_sort_by_list():
    case = vc.get_case("lists_rising")
    lod = case.lod.astype(np.int64)
    order = np.argsort(np.where(lod == vc.NO_LIST, len(case.cent), lod), kind="stable")      # the registration: (list, doc) sorted stably by list
    begin = 0
    for l in range(len(case.cent)):
        rows = vc.list_rows(case.lod, l)
        assert order[begin:begin + len(rows)].tolist() == rows.tolist() and (np.diff(rows) > 0).all()
        begin += len(rows)
    assert begin == int((lod != vc.NO_LIST).sum()) == 3840
    # the model's candidates of a query that probes list 0 alone are these rows, whatever their order in the model
    one = vc.get_case("lists_plateau")
    hits, n = vc.model_rows(one)
    assert set(hits["doc"][0, :n[0]].tolist()) <= set(vc.list_rows(one.lod, 0).tolist())
