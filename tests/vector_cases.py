"""Named cases for the candidate lists of k_vec_topk (csrc/vector.hip) and k_vec_topk_lists (csrc/vector_lists.hip), and a replay of
the kernels' list bookkeeping (csrc/vector_device.hpp) that shows which path a case reaches.  tests/test_vector_cases_cpu.py asserts
the property every case is named for from the replay; tests/test_gpu_vector_paths.py runs the cases on the device and compares bytes
with tests/vector_model.py / tests/vector_lists_model.py.  The replay is reach evidence only: expected rows never come from it.

The bookkeeping.  A query keeps up to `cap` keys in LDS behind a threshold (0 at first).  The workgroup walks its chunk of docs (a
segment of a list's rows) in rounds of WAVES * TILE = 256 positions: wave w takes positions 256 r + 64 w .. + 63 of round r, in four
steps of 16.  A position that is valid (inside the chunk, in the query's allow-list) and whose key is above the threshold is appended.
Before every round (before every step when `tight`, i.e. cap < k + 256) there is a check: a list with n + inc > cap (inc = 256, or 64
when tight: what one interval can append) is cut back to its k largest keys, and the k-th becomes the threshold.  The kernels guard the
check with a flag that the appends raise; the flag is up exactly when some list of the block has n + inc > cap, so the replay needs no
flag.  What a cut keeps is a set (an exact top k of distinct keys), so counts and thresholds do not depend on the order in which lanes
append.  Only `holes` of a list's first cut can: which keys stand in the first k slots is decided by arrival order inside one interval;
the replay returns the bounds (lo, hi) that every order respects, lo == hi from the second cut on.

Row order inside a list of ss_scorer_set_vector_lists is ascending doc id (the registration sorts (list, doc) stably by list):
list_rows() states it, and the CPU test holds it against a stable argsort of list_of_doc.

The plans come from the product's planner through tests/vector_plan_harness.cpp and tests/vector_lists_plan_harness.cpp, compiled here
with the host compiler (no sanitizer: tests/test_vector_cpu.py and tests/test_vector_lists_cpu.py run them under one), with the LDS
limit topk_impl clamps to.  Every case sets "vec.chunk_docs" / "vec.list_seg_rows", so the compute-unit count does not enter a plan.
"""
import atexit
import functools
import os
import re
import shutil
import subprocess
import tempfile
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from tests import vector_lists_model as vlm
from tests import vector_model as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spaghettisearch_amd", "csrc")
LDS_LIMIT = 160 << 10            # topk_impl: min(the device's limit, 160 KB)
N_CU = 256                       # enters only the default chunking, which no case but the control uses
NO_LIST = vlm.NO_LIST
VEC_HIT = np.dtype([("doc", "<u4"), ("score", "<i4")])


def _constant(name):
    src = open(os.path.join(CSRC, "vector_plan.hpp")).read()
    return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, src).group(1))


TILE, WAVES = _constant("TILE"), _constant("WAVES")
ROUND = TILE * WAVES             # positions of one round of the workgroup
STEP = TILE // 4                 # positions of one wave step: one 16-row A tile


# ---- the planner --------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def harnesses():
    """(vector_plan_harness, vector_lists_plan_harness) built once per process"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    out = tempfile.mkdtemp(prefix="vector_cases_")
    atexit.register(shutil.rmtree, out, ignore_errors=True)
    exes = []
    for name in ("vector_plan_harness", "vector_lists_plan_harness"):
        exe = os.path.join(out, name)
        subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", name + ".cpp"), "-o", exe], check=True)
        exes.append(exe)
    return tuple(exes)


def _run(exe, line):
    r = subprocess.run([exe], input=line + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok 1 lines", lines
    return [int(x) for x in lines[0].split()]


def _with_tight(p, k):
    assert p["ok"] == 1 and p["too_large"] == 0, p
    p["k"] = k
    p["tight"] = p["cap"] < k + ROUND                          # k_vec_topk: cap < k + VT_WAVES * VT_TILE
    p["inc"] = TILE if p["tight"] else ROUND
    return p


@functools.lru_cache(maxsize=None)
def exact_plan(n_docs, dim, n_q, k, chunk_docs):
    names = ("ok", "too_large", "q_block", "n_qblocks", "chunk_docs", "n_chunks", "cap", "row_stride", "lds_bytes", "part_keys")
    out = _run(harnesses()[0], f"{n_docs} {dim} {n_q} {k} {chunk_docs} {N_CU} {LDS_LIMIT}")
    return _with_tight(dict(zip(names, out)), k)


@functools.lru_cache(maxsize=None)
def lists_plan(lens, dim, n_q, k, n_probe, seg_rows):
    names = ("ok", "too_large", "n_probe", "seg_rows", "slots_per_q", "q_batch", "n_batches", "part_keys", "q_block", "cap", "lds_bytes", "slots")
    runs = " ".join(f"{n} 1" for n in lens)
    out = _run(harnesses()[1], f"P {dim} {n_q} {k} {n_probe} {seg_rows} 0 {N_CU} {LDS_LIMIT} {len(lens)} {runs}")
    p = _with_tight(dict(zip(names, out)), k)
    assert p["n_batches"] == 1, p
    return p


# ---- the replay ---------------------------------------------------------------------------------------------------------------------

def keys_of(score, doc):
    """vec_key: descending key order is score descending, doc ascending"""
    return (np.asarray(score, np.int64) + 2 ** 31).astype(np.uint64) << np.uint64(32) | (0xFFFFFFFF - np.asarray(doc, np.int64)).astype(np.uint64)


def rows_of(keys):
    out = np.zeros(len(keys), VEC_HIT)
    out["doc"] = 0xFFFFFFFF - (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    out["score"] = (keys >> np.uint64(32)).astype(np.int64) - 2 ** 31
    return out


@dataclass
class Replay:
    checks: list = field(default_factory=list)    # (round, step, n, cut) of every check, the first (n = 0) included
    cuts: list = field(default_factory=list)      # in-loop cuts: dict(round, step, n, holes=(lo, hi), thr, appended_since)
    end_cut: Optional[dict] = None                # the cut behind the loop, when the list ends above k
    final: Optional[np.ndarray] = None            # the chunk's keys, descending, at most k
    appended: int = 0                             # keys that passed their threshold, over the whole chunk


def _cut(batches, k):
    """batches: the list's keys in slot order, as runs whose inner order is not determined -> (kept keys, threshold, holes bounds)"""
    keys = np.concatenate(batches)
    kept = np.sort(keys)[::-1][:k]
    thr = kept[-1]
    lo = hi = 0
    room = k
    for b in batches:                                          # the first k slots: whole runs, then any `room` keys of the next run
        if room == 0:
            break
        out = int((b < thr).sum())
        if len(b) <= room:
            lo, hi = lo + out, hi + out
            room -= len(b)
        else:
            stay = len(b) - out
            lo, hi = lo + max(0, room - stay), hi + min(room, out)
            room = 0
    return kept, thr, (lo, hi)


def replay(key, valid, k, cap, tight):
    """key uint64 [n], valid bool [n]: the positions of one chunk (segment) in the kernel's order -> Replay"""
    n_pos = len(key)
    inc = TILE if tight else ROUND
    pos = np.arange(n_pos)
    rnd, step = pos // ROUND, (pos % TILE) // STEP
    rep = Replay()
    batches, n, thr, since = [], 0, np.uint64(0), 0
    for r in range(-(-n_pos // ROUND)):
        for t in range(4 if tight else 1):
            cut = n + inc > cap
            rep.checks.append((r, t, n, cut))
            if cut:
                assert n > k
                kept, thr, holes = _cut(batches, k)
                rep.cuts.append(dict(round=r, step=t, n=n, holes=holes, thr=int(thr), appended_since=since))
                batches, n, since = [kept], k, 0
            here = (rnd == r) & valid & (key > thr)
            if tight:
                here &= step == t
            new = key[here]
            assert n + len(new) <= cap                         # the kernel's `pos < cap`
            if len(new):
                batches.append(new)
                n += len(new)
                since += len(new)
                rep.appended += len(new)
    if n > k:
        kept, thr, holes = _cut(batches, k)
        rep.end_cut = dict(n=n, holes=holes, thr=int(thr))
        batches = [kept]
    rep.final = np.sort(np.concatenate(batches))[::-1] if batches else np.zeros(0, np.uint64)
    return rep


def list_rows(lod, l):
    """the docs of list l in the order of the list-major copy: ascending doc id"""
    return np.flatnonzero(np.asarray(lod) == l)


# ---- cases --------------------------------------------------------------------------------------------------------------------------

@dataclass
class Case:
    name: str
    kind: str                                     # "exact": ss_vector_topk, "lists": ss_vector_topk_probed
    vec: np.ndarray
    qvec: np.ndarray
    k: int
    options: dict                                 # library options of the call
    mask_id: Optional[np.ndarray] = None
    masks: Optional[np.ndarray] = None            # bool [n_masks][n_docs]
    cent: Optional[np.ndarray] = None
    lod: Optional[np.ndarray] = None
    n_probe: int = 1
    default_plan: bool = False                    # the control: no option, the planner's own chunking
    same_rows_as: Optional[str] = None            # a case whose rows this one must repeat byte for byte
    note: str = ""

    @property
    def plan(self):
        n_docs, dim = self.vec.shape
        if self.kind == "exact":
            return exact_plan(n_docs, dim, len(self.qvec), self.k, 0 if self.default_plan else self.options["vec.chunk_docs"])
        lens = tuple(int((self.lod == l).sum()) for l in range(len(self.cent)))
        return lists_plan(lens, dim, len(self.qvec), self.k, self.n_probe, self.options["vec.list_seg_rows"])

    def allowed(self, q):
        if self.mask_id is None or self.mask_id[q] < 0:
            return np.ones(len(self.vec), bool)
        return self.masks[self.mask_id[q]]


def replay_case(case):
    """-> {(chunk, query): Replay} for an exact case, {(query, probe rank, segment): Replay} for a list case"""
    p = case.plan
    sc = vm.scores(case.qvec, case.vec)
    docs = np.arange(len(case.vec))
    out = {}
    if case.kind == "exact":
        for c in range(p["n_chunks"]):
            lo, hi = c * p["chunk_docs"], min((c + 1) * p["chunk_docs"], len(docs))
            for q in range(len(case.qvec)):
                out[c, q] = replay(keys_of(sc[q, lo:hi], docs[lo:hi]), case.allowed(q)[lo:hi], case.k, p["cap"], p["tight"])
        return out
    pr = vlm.probes(case.qvec, case.cent, case.n_probe)
    for q in range(len(case.qvec)):
        for rank, l in enumerate(pr[q].tolist()):
            rows = list_rows(case.lod, l)
            for s in range(-(-len(rows) // p["seg_rows"])):
                seg = rows[s * p["seg_rows"]:(s + 1) * p["seg_rows"]]
                out[q, rank, s] = replay(keys_of(sc[q, seg], seg), case.allowed(q)[seg], case.k, p["cap"], p["tight"])
    return out


def merged_rows(case, reps):
    """k_vec_merge over the replay's last lists -> (hits VEC_HIT [n_q][k] zero-filled, n_hits)"""
    n_q = len(case.qvec)
    hits, n_hits = np.zeros((n_q, case.k), VEC_HIT), np.zeros(n_q, np.int32)
    q_at = 1 if case.kind == "exact" else 0
    for q in range(n_q):
        parts = [r.final for key, r in reps.items() if key[q_at] == q]
        keys = np.sort(np.concatenate(parts))[::-1][:case.k] if parts else np.zeros(0, np.uint64)
        n_hits[q] = len(keys)
        hits[q, :len(keys)] = rows_of(keys)
    return hits, n_hits


def model_rows(case):
    n_q = len(case.qvec)
    hits, n_hits = np.zeros((n_q, case.k), VEC_HIT), np.zeros(n_q, np.int32)
    if case.kind == "exact":
        vm.topk(case.qvec, case.vec, case.k, hits, n_hits, case.mask_id, case.masks)
    else:
        vlm.topk_probed(case.qvec, case.vec, case.cent, case.lod, case.k, case.n_probe, hits, n_hits, case.mask_id, case.masks)
    return hits, n_hits


# ---- tables and queries -------------------------------------------------------------------------------------------------------------
# The structured table: position 0 = doc // 64, position 1 = doc % 64, so the query (64, 1) scores a doc by its id (int8 holds one
# position only up to 127: test_chunk_seams_and_merge's single position cannot rise over 4096 docs); position 2 = 1 (a per-query
# offset, or alone the plateau), position 3 = doc // 300 (steps), positions 4 .. 15 zero (the list cases' centroids live there, so a
# query chooses its lists without moving a doc's score), positions 16 .. random.
RANDOM_FROM = 16


def table(n_docs, seed, dim=64):
    assert n_docs <= 127 * 64
    rng = np.random.default_rng(seed)
    vec = rng.integers(-128, 128, (n_docs, dim)).astype(np.int8)
    d = np.arange(n_docs)
    vec[:, 0], vec[:, 1], vec[:, 2], vec[:, 3] = d // 64, d % 64, 1, d // 300
    vec[:, 4:RANDOM_FROM] = 0
    return rng, vec


def q_rising(off=0, dim=64):
    q = np.zeros(dim, np.int8)
    q[0], q[1], q[2] = 64, 1, off
    return q


def q_falling(off=0, dim=64):
    q = np.zeros(dim, np.int8)
    q[0], q[1], q[2] = -64, -1, off
    return q


def q_plateau(off=5, dim=64):
    q = np.zeros(dim, np.int8)
    q[2] = off
    return q


def q_steps(dim=64):
    q = np.zeros(dim, np.int8)
    q[3] = 1
    return q


def q_random(rng, dim=64):
    q = np.zeros(dim, np.int8)
    q[RANDOM_FROM:] = rng.integers(-128, 128, dim - RANDOM_FROM)
    return q


def mixed_queries(rng, n_q):
    kinds = (lambda i: q_rising(i % 100), lambda i: q_random(rng), lambda i: q_falling(i % 100))
    return np.stack([kinds[i % 3](i) for i in range(n_q)])


N_DOCS = 4096


def _exact(name, vec, qvec, k, chunk=None, **kw):
    return Case(name, "exact", vec, qvec, k, {"vec.chunk_docs": len(vec) if chunk is None else chunk}, **kw)


def _rising(chunk=None, name="rising", **kw):
    _, vec = table(N_DOCS, 101)
    return _exact(name, vec, np.stack([q_rising(o) for o in range(17)]), 10, chunk, **kw)


def _falling():
    # queries 0 .. 15 plain; query 16 may take docs 0 .. k - 1 of round 0 and every doc from round 1 on: at its cut the first k slots
    # hold exactly its k best docs, whatever the order of arrival: holes == 0
    _, vec = table(N_DOCS, 102)
    masks = np.ones((1, N_DOCS), bool)
    masks[0, 10:ROUND] = False
    mask_id = np.full(17, -1, np.int32)
    mask_id[16] = 0
    return _exact("falling", vec, np.stack([q_falling(o) for o in range(17)]), 10, mask_id=mask_id, masks=masks)


def _plateau():
    _, vec = table(N_DOCS, 103)
    return _exact("plateau", vec, np.stack([q_plateau(), q_steps()]), 10)


def _exact_fill():
    # query 0: cap - 256 docs of round 0, all of round 1: n + inc == cap at the check between them, n == cap at the next
    rng, vec = table(N_DOCS, 104)
    qvec = np.stack([q_rising(o) for o in range(17)])
    cap = exact_plan(N_DOCS, 64, 17, 10, N_DOCS)["cap"]
    assert 0 < cap - ROUND <= ROUND and cap >= 10 + ROUND, cap
    masks = np.ones((1, N_DOCS), bool)
    masks[0, :ROUND] = False
    masks[0, np.sort(rng.choice(ROUND, cap - ROUND, replace=False))] = True
    mask_id = np.full(17, -1, np.int32)
    mask_id[0] = 0
    return _exact("exact_fill", vec, qvec, 10, mask_id=mask_id, masks=masks)


def _mixed_block():
    # one block of 17: 0 .. 5 rising, 6 .. 10 falling, 11 and 14 .. 16 random, 12 with 7 docs in its allow-list, 13 with none
    rng, vec = table(N_DOCS, 105)
    qvec = np.stack([q_rising(i) for i in range(6)] + [q_falling(i) for i in range(5)] + [q_random(rng), q_rising(3), q_rising(4)]
                    + [q_random(rng) for _ in range(3)])
    masks = np.zeros((2, N_DOCS), bool)
    masks[0, [3, 255, 256, 1000, 2047, 2048, 4095]] = True
    mask_id = np.full(17, -1, np.int32)
    mask_id[12], mask_id[13] = 0, 1
    return _exact("mixed_block", vec, qvec, 10, mask_id=mask_id, masks=masks)


def _masked_winners():
    # 2080 docs: 65 mask words, so the last tile's second word does not exist; two chunks of 1088 and 992 docs
    n_docs, chunk, k = 2080, 1088, 10
    rng, vec = table(n_docs, 106)
    masks = rng.random((3, n_docs)) < 0.5
    for end in (chunk, n_docs):
        masks[:, end - 2 * k:end] = False                      # the 2k best docs of each chunk under a rising query
    mask_id = (np.arange(17) % 4 - 1).astype(np.int32)         # -1, 0, 1, 2, ...
    assert -(-n_docs // 32) % 2 == 1
    return _exact("masked_winners", vec, np.stack([q_rising(o) for o in range(17)]), k, chunk, mask_id=mask_id, masks=masks)


def _tight100(chunk=None, name="tight_k100", **kw):
    # 33 queries: a block of 32 and a block of 1; rising, random and falling queries
    rng, vec = table(N_DOCS, 107)
    return _exact(name, vec, mixed_queries(rng, 33), 100, chunk, **kw)


def _tight1024(chunk=None, name="tight_k1024", **kw):
    rng, vec = table(N_DOCS, 108)
    return _exact(name, vec, np.stack([q_rising(0), q_rising(7), q_random(rng)]), 1024, chunk, **kw)


def _query_blocks(n_q):
    rng, vec = table(N_DOCS, 109)
    return _exact(f"query_blocks_{n_q}", vec, mixed_queries(rng, n_q), 10)


def _random(k):
    rng = np.random.default_rng(110)
    vec = rng.integers(-128, 128, (N_DOCS, 64)).astype(np.int8)
    return _exact(f"random_k{k}", vec, rng.integers(-128, 128, (5, 64)).astype(np.int8), k)


def _control():
    # test_gpu_vector.py's test_shapes (4099, 64, 17, 10), its data and the default plan
    n_docs, dim, n_q, k = 4099, 64, 17, 10
    rng = np.random.default_rng(n_docs * 7 + dim + n_q + k)
    vec = rng.integers(-128, 128, (n_docs, dim)).astype(np.int8)
    qvec = rng.integers(-128, 128, (n_q, dim)).astype(np.int8)
    return Case("control_default_plan", "exact", vec, qvec, k, {}, default_plan=True)


# ---- list cases: list 0 holds 2304 docs (doc % 16 < 9), list 1 1024, list 2 512, 256 docs are in no list; centroid l is 100 at
# position 4 + l, so a query with 100 there probes list l first
LIST_OF_RESIDUE = [0] * 9 + [1] * 4 + [2] * 2 + [NO_LIST]
ONE_SEGMENT = 4096                                             # "vec.list_seg_rows": list 0 is one segment


def list_world(seed):
    rng, vec = table(N_DOCS, seed)
    lod = np.array(LIST_OF_RESIDUE, np.uint32)[np.arange(N_DOCS) % 16]
    cent = np.zeros((3, 64), np.int8)
    cent[np.arange(3), 4 + np.arange(3)] = 100
    return rng, vec, cent, lod


def on_list(qvec, l=0):
    qvec = np.array(qvec)
    qvec[:, 4 + l] = 100
    return qvec


def _lists(name, world, qvec, k, seg=ONE_SEGMENT, **kw):
    _, vec, cent, lod = world
    return Case(name, "lists", vec, qvec, k, {"vec.list_seg_rows": seg}, cent=cent, lod=lod, **kw)


def _l_rising(seg=ONE_SEGMENT, name="lists_rising", **kw):
    w = list_world(201)
    return _lists(name, w, on_list(np.stack([q_rising(o) for o in range(17)])), 10, seg, **kw)


def _l_falling():
    w = list_world(202)
    rows = list_rows(w[3], 0)
    masks = np.ones((1, N_DOCS), bool)
    masks[0, rows[10:ROUND]] = False                           # _falling's allow-list, in rows of list 0
    mask_id = np.full(17, -1, np.int32)
    mask_id[16] = 0
    return _lists("lists_falling", w, on_list(np.stack([q_falling(o) for o in range(17)])), 10, mask_id=mask_id, masks=masks)


def _l_plateau():
    return _lists("lists_plateau", list_world(203), on_list(np.stack([q_plateau(), q_steps()])), 10)


def _l_mixed():
    # 19 queries on list 0, one group: 17 without an allow-list (rising, random, falling), one with 7 docs of the list, one with none
    w = list_world(204)
    rng, rows = w[0], list_rows(w[3], 0)
    qvec = np.concatenate([mixed_queries(rng, 17), np.stack([q_rising(1), q_rising(2)])])
    masks = np.zeros((2, N_DOCS), bool)
    masks[0, rows[[0, 255, 256, 1000, 2000, 2302, 2303]]] = True
    masks[0, list_rows(w[3], 1)] = True                        # (docs of a list the query does not probe)
    masks[1, list_rows(w[3], 2)] = True
    mask_id = np.full(19, -1, np.int32)
    mask_id[17], mask_id[18] = 0, 1
    return _lists("lists_mixed_block", w, on_list(qvec), 10, mask_id=mask_id, masks=masks)


def _l_tight100():
    w = list_world(205)
    return _lists("lists_tight_k100", w, on_list(mixed_queries(w[0], 33)), 100)


BUILDERS = {
    "rising": _rising,
    "falling": _falling,
    "plateau": _plateau,
    "exact_fill": _exact_fill,
    "mixed_block": _mixed_block,
    "masked_winners": _masked_winners,
    "tight_k100": _tight100,
    "tight_k1024": _tight1024,
    "rising_two_chunks": lambda: _rising(N_DOCS // 2, "rising_two_chunks", same_rows_as="rising"),
    "tight_k100_two_chunks": lambda: _tight100(N_DOCS // 2, "tight_k100_two_chunks", same_rows_as="tight_k100"),
    "tight_k1024_two_chunks": lambda: _tight1024(N_DOCS // 2, "tight_k1024_two_chunks", same_rows_as="tight_k1024"),
    "query_blocks_64": lambda: _query_blocks(64),
    "query_blocks_65": lambda: _query_blocks(65),
    "query_blocks_130": lambda: _query_blocks(130),
    "random_k1": lambda: _random(1),
    "random_k10": lambda: _random(10),
    "random_k100": lambda: _random(100),
    "random_k1024": lambda: _random(1024),
    "lists_rising": _l_rising,
    "lists_falling": _l_falling,
    "lists_plateau": _l_plateau,
    "lists_mixed_block": _l_mixed,
    "lists_tight_k100": _l_tight100,
    "lists_two_segments": lambda: _l_rising(1152, "lists_two_segments", same_rows_as="lists_rising"),
}
CASE_NAMES = list(BUILDERS)                                    # the cases the device runs
CONTROL = "control_default_plan"                               # CPU only: test_gpu_vector.py runs that shape itself


@functools.lru_cache(maxsize=None)
def get_case(name):
    case = _control() if name == CONTROL else BUILDERS[name]()
    assert case.name == name
    return case
