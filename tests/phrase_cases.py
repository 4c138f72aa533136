"""Constructed inputs for the quoted-phrase path (k_phrase_match / k_phrase_close and their host plan in csrc/score_call.hip).

Every table is built from explicit per-term doc sets and position lists, so the phrase's driver (its rarest term, whose
postings are the candidates), the driver's list lengths, the split of the candidates into workgroup parts of PH_PART and
which candidate matches are known by construction.  Each query carries the condition it is meant to hit as data (`claim`);
tests/test_phrase_cases_cpu.py proves the claims from tests/phrase_model.py and holds the C oracle against that model,
tests/test_gpu_phrase_edges.py runs the same cases on the device.

Families (the letter starts the case name):
  A  part seams: driver body lists of 1 .. 16385 candidates, five match patterns each
  B  close-up with overlapping source and destination: part 0 short of g matches, the later parts full
  C  pass 1 (the driver's title postings): a driver without body postings, a driver in both fields
  D  field mixing of phrase.go:63-92
  E  position lists: empty, only -100, unsorted, duplicated, long, at and above 2^24
  F  phrase lengths 1 / 2 / 15 / 16 (17: an error), repeated terms, the order of the float32 weight sum
  G  one table with parts of all of them, for mixed batches

Weights are multiples of 1/64 in [3/64, 1] that differ from doc to doc (a row that lands in the wrong slot shows), except the
2^24, 1, 1 triple of family F; magnitudes are the float64 l2 norms of the float32 weights (1 for a doc without postings).
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from tests.phrase_model import PhraseModel

PH_PART = 8192          # candidates per k_phrase_match workgroup
PH_TPB = 256            # threads of a workgroup = rows k_phrase_close moves per step
PH_MAX = 16             # SS_MAX_PHRASE_TERMS
TITLE, BODY = 0, 1

Query = namedtuple("Query", "name terms phrase claim")


class Tables:
    """Collects postings (field, term, doc, weight, positions) and lays them out as the two CSR tables."""

    def __init__(self):
        self.pieces = {TITLE: {}, BODY: {}}

    def add(self, field, term, docs, w, pos):
        """pos: an array [n][c] (c positions for every posting) or a list of n sequences."""
        docs = np.asarray(docs, dtype=np.int64).ravel()
        w = np.broadcast_to(np.asarray(w, dtype=np.float32), docs.shape).copy()
        if isinstance(pos, np.ndarray) and pos.ndim == 2:
            cnt = np.full(len(docs), pos.shape[1], dtype=np.int64)
            flat = pos.astype(np.float32).ravel()
        else:
            assert len(pos) == len(docs)
            cnt = np.array([len(p) for p in pos], dtype=np.int64)
            flat = np.array([x for p in pos for x in p], dtype=np.float32)
        assert len(cnt) == len(docs) and int(cnt.sum()) == len(flat)
        self.pieces[field].setdefault(int(term), []).append((docs, w, cnt, flat))

    def _finish_field(self, field, n_docs, n_terms):
        ptr, doc_l, w_l, cnt_l, pos_l = [0], [], [], [], []
        for t in range(n_terms):
            ps = self.pieces[field].get(t, [])
            if ps:
                docs, w, cnt, flat = (np.concatenate([p[i] for p in ps]) for i in range(4))
                order = np.argsort(docs, kind="stable")
                assert (np.diff(docs[order]) > 0).all(), (field, t)          # one posting per (term, doc)
                assert docs.min() >= 0 and docs.max() < n_docs, (field, t)
                start = np.concatenate([[0], np.cumsum(cnt)])[:-1]
                c2 = cnt[order]
                new_start = np.concatenate([[0], np.cumsum(c2)])[:-1]
                idx = np.repeat(start[order] - new_start, c2) + np.arange(int(c2.sum()))
                doc_l.append(docs[order])
                w_l.append(w[order])
                cnt_l.append(c2)
                pos_l.append(flat[idx])
            ptr.append(ptr[-1] + (len(ps) and sum(len(p[0]) for p in ps)))
        assert not set(self.pieces[field]) - set(range(n_terms))
        cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
        table = (np.array(ptr, dtype=np.uint64), cat(doc_l, np.uint32), cat(w_l, np.float32))
        pos = (np.concatenate([[0], np.cumsum(cat(cnt_l, np.int64))]).astype(np.uint64), cat(pos_l, np.float32))
        sq = (table[2] * table[2]).astype(np.float32).astype(np.float64)
        mag = np.sqrt(np.bincount(table[1].astype(np.int64), weights=sq, minlength=n_docs))
        mag[mag == 0] = 1.0
        return table, pos, mag

    def finish(self, n_docs, n_terms):
        return self._finish_field(TITLE, n_docs, n_terms), self._finish_field(BODY, n_docs, n_terms)


class PhraseCase:
    def __init__(self, name, tables, n_docs, n_terms, queries, errors=()):
        self.name, self.family = name, name[0]
        self.n_docs, self.n_terms = int(n_docs), int(n_terms)
        (self.title, self.tpos, self.mag_t), (self.body, self.bpos, self.mag_b) = tables.finish(n_docs, n_terms)
        self.queries = list(queries)
        self.errors = list(errors)                       # queries the library must refuse: claim["code"]
        assert len({q.name for q in self.queries}) == len(self.queries)
        self._model = None
        self._results = {}

    def model(self):
        if self._model is None:
            self._model = PhraseModel(self.title, self.body, self.tpos, self.bpos)
        return self._model

    def model_phrase(self, phrase):
        """The model's (docs, title_sum, body_sum, flags) of one phrase (computed once, handed out read-only)."""
        key = tuple(int(t) for t in phrase)
        if key not in self._results:
            r = self.model().phrase(list(key))
            for a in r:
                a.setflags(write=False)
            self._results[key] = r
        return self._results[key]

    def extra(self, q):
        """What oracle.score_topk takes as `extra` for this query: None without a phrase."""
        return self.model_phrase(q.phrase) if len(q.phrase) else None

    def df(self, term):
        return (int(self.body[0][term + 1]) - int(self.body[0][term]), int(self.title[0][term + 1]) - int(self.title[0][term]))

    def driver(self, phrase):
        """The host plan's rule: the phrase term with the smallest title + body document frequency, the first of equals.
        -> (slot, term, body list length, title list length), or None when a term is unknown (no candidates at all)."""
        best = None
        for i, t in enumerate(phrase):
            if int(t) >= self.n_terms:
                return None
            nb, nt = self.df(int(t))
            if best is None or nb + nt < best[2] + best[3]:
                best = (i, int(t), nb, nt)
        return best

    def runs(self, phrase):
        """What k_phrase_close has to move for this phrase, from the model's matches and the driver's lists alone: one entry per
        (pass, result kind, part) = dict(pas, kind, part, n = matches of the part, gap = src - dst = candidates before the part
        that gave no record of this kind).  Pass 1 skips docs that hold the driver in the body: they are non-matches there."""
        drv = self.driver(phrase)
        if drv is None:
            return []
        docs, _, _, flags = self.model_phrase(phrase)
        flag_of = np.zeros(self.n_docs, dtype=np.uint8)
        flag_of[docs.astype(np.int64)] = flags
        _, term, _, _ = drv
        body_docs = self.body[1][int(self.body[0][term]):int(self.body[0][term + 1])].astype(np.int64)
        title_docs = self.title[1][int(self.title[0][term]):int(self.title[0][term + 1])].astype(np.int64)
        in_body = np.zeros(self.n_docs, dtype=bool)
        in_body[body_docs] = True
        out = []
        for pas, cand in ((0, body_docs), (1, title_docs)):
            for kind, bit in (("body", 2), ("title", 1)):
                hit = (flag_of[cand] & bit) != 0
                if pas == 1:
                    hit &= ~in_body[cand]
                before = 0
                for part, c0 in enumerate(range(0, len(cand), PH_PART)):
                    n = int(hit[c0:c0 + PH_PART].sum())
                    out.append(dict(pas=pas, kind=kind, part=part, n=n, gap=c0 - before, first=c0))
                    before += n
        return out


def wt(docs, salt):
    """float32 weights k / 64, k in 3 .. 63, that change from doc to doc."""
    return (((np.asarray(docs, dtype=np.int64) * 7 + salt) % 61 + 3) / 64.0).astype(np.float32)


def col(n, *values):
    """[n][len(values)] positions, the same list for every posting."""
    return np.tile(np.array(values, dtype=np.float32), (n, 1))


# ---- emitters: each writes its postings from doc d0 / term t0 on and returns (docs used, terms used, queries) ----------------

def emit_driver_patterns(tb, d0, t0, L, patterns, family, tag):
    """A driver (term t0) with L body postings and no title posting, docs d0 + 3 .. d0 + L + 2 with positions [5, 40]; per pattern
    a partner term on the same docs and on d0 .. d0 + 2 (so the partner is never the rarer term), whose positions chain with
    the driver's where the pattern says so.  Odd-numbered patterns put the driver in slot 1: "partner driver".  Term t0 + 1 +
    len(patterns) is a plain word on every third doc (body) and every seventh (title) for OR terms beside the phrase."""
    cand = d0 + 3 + np.arange(L)
    extra = d0 + np.arange(3)
    tb.add(BODY, t0, cand, wt(cand, 1), col(L, 5, 40))
    queries = []
    filler = t0 + 1 + len(patterns)
    for i, (pname, match) in enumerate(patterns.items()):
        assert match.shape == (L,) and match.dtype == np.bool_
        partner = t0 + 1 + i
        reverse = i % 2 == 1
        pos = col(L, 2, 7) if not reverse else col(L, 3, 30)            # 7 - 1 and 2 - 1 miss 5 and 40; 5 - 1 and 40 - 1 miss 3 and 30
        pos[match, 1 if not reverse else 0] = 6 if not reverse else 4   # 6 - 1 == 5; 5 - 1 == 4
        tb.add(BODY, partner, cand, wt(cand, 11 + i), pos)
        tb.add(BODY, partner, extra, wt(extra, 11 + i), col(3, 6) if not reverse else col(3, 4))
        claim = dict(family=family, driver=t0, slot=1 if reverse else 0, body_len=L, title_len=0, n_match=int(match.sum()), pattern=pname)
        if family == "B":               # src - dst of every part behind part 0
            claim["gap"] = PH_PART if pname == "part0empty" else 0 if pname == "allfull" else int(pname[1:].split(".")[0])
        queries.append(Query(f"{tag}.{pname}", [filler] if i % 3 == 0 else [], [partner, t0] if reverse else [t0, partner], claim))
    every3 = d0 + np.arange(0, L + 3, 3)
    every7 = d0 + np.arange(0, L + 3, 7)
    tb.add(BODY, filler, every3, wt(every3, 5), col(len(every3), 1))
    tb.add(TITLE, filler, every7, wt(every7, 6), col(len(every7), 0))
    return L + 3, len(patterns) + 2, queries


def seam_patterns(L):
    c = np.arange(L)
    return {"all": np.ones(L, dtype=bool),
            "first": c % PH_PART == 0,
            "last": (c % PH_PART == PH_PART - 1) | (c == L - 1),
            "verylast": c == L - 1,
            "none": np.zeros(L, dtype=bool)}


B_GAPS = (1, 255, 256, 257)


def overlap_patterns(L):
    """Part 0 short of g matches at its start / middle / end, the later parts full; part 0 empty; every part full."""
    c = np.arange(L)
    out = {}
    for g in B_GAPS:
        out[f"g{g}.start"] = ~(c < g)
        out[f"g{g}.mid"] = ~((c >= 4000) & (c < 4000 + g))
        out[f"g{g}.end"] = ~((c >= PH_PART - g) & (c < PH_PART))
    out["part0empty"] = c >= PH_PART
    out["allfull"] = np.ones(L, dtype=bool)
    return out


def emit_title_only_driver(tb, d0, t0, n=8500):
    """Pass 0 has no part: the driver (t0) has n > PH_PART title postings and no body posting.  The partner holds every driver
    doc in the title (+ 5 more docs) and some of them in the body, which cannot complete the body field."""
    cand = d0 + 2 + np.arange(n)
    c = np.arange(n)
    match = (c % 3 == 0) | ((c >= PH_PART) & (c % 2 == 1))
    tb.add(TITLE, t0, cand, wt(cand, 2), col(n, 0, 9))
    pos = col(n, 3, 20)
    pos[match, 0] = 1                                                    # 1 - 1 == 0
    tb.add(TITLE, t0 + 1, cand, wt(cand, 3), pos)
    more = np.concatenate([d0 + np.arange(2), d0 + 2 + n + np.arange(3)])
    tb.add(TITLE, t0 + 1, more, wt(more, 3), col(5, 1))
    some = cand[::5]
    tb.add(BODY, t0 + 1, some, wt(some, 4), col(len(some), 1))
    claim = dict(family="C", driver=t0, slot=0, body_len=0, title_len=n, n_match=int(match.sum()), both_fields=False)
    return n + 5, 2, [Query("title_only", [], [t0, t0 + 1], claim), Query("title_only.or", [t0 + 1], [t0, t0 + 1], claim)]


def emit_both_field_driver(tb, d0, t0, n_title=9000):
    """The driver (t0) in the title of B = d0 .. d0 + n_title - 1 and in the body of A = 300 docs inside B (every 17th) + 200 docs
    behind B.  |B \\ A| > PH_PART.  The docs of A and B hold the partner in the same field(s) (+ 3 more docs per field)."""
    B = d0 + np.arange(n_title)
    A_in = d0 + 17 * np.arange(300)
    A_out = d0 + n_title + np.arange(200)
    A = np.concatenate([A_in, A_out])
    assert A_in.max() < d0 + PH_PART and n_title - len(A_in) > PH_PART
    tb.add(TITLE, t0, B, wt(B, 7), col(n_title, 2, 11))
    tb.add(BODY, t0, A, wt(A, 8), col(len(A), 4))
    ib = np.arange(n_title)
    t_match = (ib % 2 == 0) | (ib >= n_title - 100)
    pos = col(n_title, 5, 30)
    pos[t_match, 1] = 12                                                 # 12 - 1 == 11
    tb.add(TITLE, t0 + 1, B, wt(B, 9), pos)
    ia = np.arange(len(A))
    b_match = ia % 3 != 0
    pos = col(len(A), 9)
    pos[b_match, 0] = 5                                                  # 5 - 1 == 4
    tb.add(BODY, t0 + 1, A, wt(A, 10), pos)
    more = d0 + n_title + 200 + np.arange(3)
    tb.add(TITLE, t0 + 1, more, wt(more, 9), col(3, 12))
    tb.add(BODY, t0 + 1, more, wt(more, 10), col(3, 5))
    claim = dict(family="C", driver=t0, slot=0, body_len=len(A), title_len=n_title, both_fields=True,
                 n_match=int(len(np.union1d(B[t_match], A[b_match]))))
    return n_title + 203, 2, [Query("both_fields", [], [t0, t0 + 1], claim), Query("both_fields.or", [t0], [t0, t0 + 1], claim)]


def emit_field_mixing(tb, d0, t0):
    """phrase.go:63-92 on purpose, four docs per situation, phrases "a b" and "a b c" (c chains wherever it stands, so both
    phrases have the same answer).  claim["flags"]: doc -> expected record flags (bit 0 title, bit 1 body); 0 = no match."""
    a, b, c = t0, t0 + 1, t0 + 2
    flags = {}
    d = d0

    def put(field, term, doc, p):
        tb.add(field, term, [doc], wt([doc], 20 + 3 * field + term - t0), [p])

    for _ in range(4):                  # a in the body only, b in the title only: every term present, no field complete
        put(BODY, a, d, [1]); put(TITLE, b, d, [2]); put(BODY, c, d, [3]); put(TITLE, c, d, [3])
        flags[d] = 0
        d += 1
    for _ in range(4):                  # every term in the title, only a (and c) in the body: a title record of title weights
        put(TITLE, a, d, [1]); put(TITLE, b, d, [2]); put(TITLE, c, d, [3]); put(BODY, a, d, [1]); put(BODY, c, d, [3])
        flags[d] = 1
        d += 1
    for _ in range(4):                  # both fields complete, only the body chains
        put(TITLE, a, d, [1]); put(TITLE, b, d, [5]); put(TITLE, c, d, [3]); put(BODY, a, d, [7]); put(BODY, b, d, [8]); put(BODY, c, d, [9])
        flags[d] = 2
        d += 1
    for _ in range(4):                  # both fields complete, only the title chains
        put(TITLE, a, d, [1]); put(TITLE, b, d, [2]); put(TITLE, c, d, [3]); put(BODY, a, d, [7]); put(BODY, b, d, [7]); put(BODY, c, d, [9])
        flags[d] = 1
        d += 1
    for _ in range(4):                  # both chain: two records for one doc
        put(TITLE, a, d, [1]); put(TITLE, b, d, [2]); put(TITLE, c, d, [3]); put(BODY, a, d, [7]); put(BODY, b, d, [8]); put(BODY, c, d, [9])
        flags[d] = 3
        d += 1
    claim = dict(family="D", flags=flags)
    return d - d0, 3, [Query("ab", [], [a, b], claim), Query("abc", [], [a, b, c], claim), Query("ab.or", [c, a], [a, b], claim)]


_P24, _P25 = 2.0 ** 24, 2.0 ** 25
_LONG0 = [3.0 * j for j in range(300)]                                  # multiples of 3
_LONG1 = [3.0 * j + 2 for j in range(299)] + [3.0 * 299 + 1]            # x - 1 = 1 (mod 3) but for the last: 897 = _LONG0[-1]
_LONG2 = [3.0 * j + 1 for j in range(299)] + [3.0 * 299 + 2]            # x - 2 = 2 (mod 3) but for the last: 897
# (positions of term 0, 1, 2) -> does "t0", "t0 t1", "t0 t1 t2" match in a field holding these lists?  Worked out by hand from
# getPosTerm's float32 shift and intersect; the float32 cases: 2^24 + 2 - 1 = 2^24 + 1 is a tie and rounds to the even 2^24;
# 2^25 - 1 is a tie between 2^25 - 2 and 2^25 and rounds to 2^25, 2^25 - 2 is exact; 2^25 + 4 - 1 rounds to the nearer
# 2^25 + 4, 2^25 + 4 - 2 is a tie between 2^25 and 2^25 + 4 and rounds to the even 2^25.
SITUATIONS = [
    ("empty0", ([], [1], [2]), (False, False, False)),
    ("empty1", ([0], [], [2]), (True, False, False)),
    ("empty2", ([0], [1], []), (True, True, False)),
    ("anchors", ([-100], [-100], [-100]), (True, False, False)),        # -100 against -100: -101 is not -100
    ("anchor_chain", ([-100], [-99], [-98]), (True, True, True)),       # -99 - 1 = -100
    ("anchor_twice", ([-100, -100], [-99], [7]), (True, True, False)),
    ("unsorted", ([9, 3, 7], [8, 1, 4], [2, 5]), (True, True, True)),   # {7, 0, 3} meets {9, 3, 7} in 3 and 7; {0, 3} keeps 3
    ("unsorted_miss", ([9, 3, 7], [5, 6, 1], [5, 9]), (True, False, False)),
    ("duplicates", ([4, 4, 4], [5, 5], [6, 6, 6, 6]), (True, True, True)),
    ("duplicates_miss", ([4, 4], [4, 4], [4]), (True, False, False)),
    ("long_last", (_LONG0, _LONG1, _LONG2), (True, True, True)),        # 300 positions each, the chain closes at the last ones
    ("long_miss", (_LONG0, _LONG1[:-1], _LONG2), (True, False, False)),
    ("p24_exact", ([_P24], [_P24], [_P24 + 2]), (True, False, False)),  # 2^24 - 1 is representable
    ("p24_rounds", ([_P24], [_P24 + 2], [_P24 + 2]), (True, True, True)),
    ("p25_same", ([_P25], [_P25], [_P25]), (True, True, False)),        # two 2^25 entries "match"; the third gives 2^25 - 2
    ("p25_plus4", ([_P25 + 4], [_P25 + 4], [_P25 + 4]), (True, True, False)),
    ("p25_apart", ([_P25], [_P25 + 4], [_P25 + 4]), (True, False, False)),
]


def emit_positions(tb, d0, t0):
    """Doc d0 + s holds situation s in the body and situation s + 1 (cyclically) in the title, all three terms in both fields."""
    n = len(SITUATIONS)
    expect = {m: {} for m in (1, 2, 3)}                                 # phrase length -> doc -> flags
    for s in range(n):
        doc = d0 + s
        for field, sit in ((BODY, SITUATIONS[s]), (TITLE, SITUATIONS[(s + 1) % n])):
            for i in range(3):
                tb.add(field, t0 + i, [doc], wt([doc], 30 + 3 * field + i), [sit[1][i]])
            for m in (1, 2, 3):
                expect[m][doc] = expect[m].get(doc, 0) | ((2 if field == BODY else 1) if sit[2][m - 1] else 0)
    qs = [Query(f"len{m}", [], [t0 + i for i in range(m)], dict(family="E", flags=expect[m])) for m in (1, 2, 3)]
    qs.append(Query("len2.or", [t0 + 2], [t0, t0 + 1], dict(family="E", flags=expect[2])))
    return n, 3, qs


def emit_lengths(tb, d0, t0):
    """16 terms u_i at position 10 + i (and a stray 50 - i) in docs d0 .. d0 + 5, the title too in the first three; doc d0 + 4 has
    u_15 off by one, doc d0 + 5 lacks u_14.  A word at [3, 4] / [3] / [4, 3] / [3, 5] for "a a", with b at [4] for "a b a".  The
    weights 2^24, 1, 1 of x, y, z with positions that chain in all three rotations of "x y z"; x is the rarest of the three."""
    u = [t0 + i for i in range(PH_MAX)]
    for i, t in enumerate(u):
        docs = [d0 + j for j in range(6) if not (i == 14 and j == 5)]
        pos = [[50 - i, 10 + i + (1 if (i == 15 and d == d0 + 4) else 0)] for d in docs]
        tb.add(BODY, t, docs, wt(docs, 40 + i), pos)
        tb.add(TITLE, t, docs[:3], wt(docs[:3], 60 + i), pos[:3])
    flags_all = {d0: 3, d0 + 1: 3, d0 + 2: 3, d0 + 3: 2, d0 + 4: 2, d0 + 5: 2}
    queries = [Query("len1", [], u[:1], dict(family="F", flags=dict(flags_all))),
               Query("len2", [u[3]], u[:2], dict(family="F", flags=dict(flags_all))),
               Query("len15", [], u[:15], dict(family="F", flags={d: f for d, f in flags_all.items() if d != d0 + 5})),
               Query("len16", [], u[:16], dict(family="F", flags={d: f for d, f in flags_all.items() if d < d0 + 4}))]
    errors = [Query("len17", [], u + [u[0]], dict(family="F", code=7))]
    a, b = t0 + 16, t0 + 17
    da = [d0 + 6 + j for j in range(4)]
    tb.add(BODY, a, da, wt(da, 80), [[3, 4], [3], [4, 3], [3, 5]])
    tb.add(BODY, b, da, wt(da, 81), [[4]] * 4)
    queries.append(Query("aa", [], [a, a], dict(family="F", flags={da[0]: 2, da[2]: 2})))
    queries.append(Query("aba", [], [a, b, a], dict(family="F", flags={da[3]: 2})))
    x, y, z = t0 + 18, t0 + 19, t0 + 20
    dx = [d0 + 10 + j for j in range(5)]
    for field in (TITLE, BODY):
        tb.add(field, x, dx, np.float32(2.0 ** 24), [[10, 22, 31]] * 5)
        tb.add(field, y, dx + [d0 + 15, d0 + 16], np.float32(1.0), [[11, 20, 32]] * 7)
        tb.add(field, z, dx + [d0 + 15, d0 + 17], np.float32(1.0), [[12, 21, 30]] * 7)
    triple = {d: 3 for d in dx}
    for order, slot in (((x, y, z), 0), ((y, z, x), 2), ((z, x, y), 1)):
        queries.append(Query("order." + "xyz"[(3 - slot) % 3:] + "xyz"[:(3 - slot) % 3], [], list(order),
                             dict(family="F", flags=dict(triple), driver=x, slot=slot, order=True)))
    return 18, 21, queries, errors


# ---- the cases -------------------------------------------------------------------------------------------------------------------

A_LENGTHS = (1, 255, 256, 257, 8191, 8192, 8193, 16384, 16385)
B_LENGTHS = (16384, 24576)


def _prefixed(queries, prefix):
    return [q._replace(name=f"{prefix}.{q.name}") for q in queries]


def _case_a(L):
    tb = Tables()
    n_docs, n_terms, qs = emit_driver_patterns(tb, 0, 0, L, seam_patterns(L), "A", f"A.L{L}")
    return PhraseCase(f"A.L{L}", tb, n_docs, n_terms, qs)


def _case_b(L):
    tb = Tables()
    n_docs, n_terms, qs = emit_driver_patterns(tb, 0, 0, L, overlap_patterns(L), "B", f"B.L{L}")
    return PhraseCase(f"B.L{L}", tb, n_docs, n_terms, qs)


def _case_c(which):
    tb = Tables()
    n_docs, n_terms, qs = (emit_title_only_driver if which == "title_only" else emit_both_field_driver)(tb, 0, 0)
    return PhraseCase(f"C.{which}", tb, n_docs, n_terms, _prefixed(qs, "C"))


def _case_small(name, emit):
    tb = Tables()
    out = emit(tb, 0, 0)
    return PhraseCase(name, tb, out[0], out[1], _prefixed(out[2], name), _prefixed(out[3], name) if len(out) > 3 else ())


def _case_g():
    """Parts of the families A-F in one table, so one batch can hold phrases with 0, 1, 2 and 3 parts, plain OR queries, the same
    phrase twice and a phrase with an unknown word.  claim["family"] stays the source family's."""
    tb = Tables()
    d0 = t0 = 0
    queries, errors = [], []
    L, LB = PH_TPB + 1, 2 * PH_PART
    pats, pats_b = seam_patterns(L), overlap_patterns(LB)
    for prefix, emit in (("A", lambda tb, d, t: emit_driver_patterns(tb, d, t, L, {k: pats[k] for k in ("all", "last")}, "A", f"L{L}")),
                         ("B", lambda tb, d, t: emit_driver_patterns(tb, d, t, LB, {k: pats_b[k] for k in ("g255.mid", "g1.start")}, "B", f"L{LB}")),
                         ("C", emit_both_field_driver), ("D", emit_field_mixing), ("E", emit_positions), ("F", emit_lengths)):
        out = emit(tb, d0, t0)
        queries += _prefixed(out[2], f"G.{prefix}")
        if len(out) > 3:
            errors += _prefixed(out[3], f"G.{prefix}")
        d0 += out[0]
        t0 += out[1]
    by = {q.name: q for q in queries}
    plain = [Query("G.or1", [2], [], dict(family="G")), Query("G.or3", [by["G.D.ab"].phrase[0], 2, by["G.E.len1"].phrase[0]], [], dict(family="G"))]
    twice = by["G.C.both_fields"]._replace(name="G.C.both_fields.again")
    unknown = [Query("G.unknown", [2], [by["G.C.both_fields"].phrase[0], t0 + 5], dict(family="G", unknown=True)),
               Query("G.unknown_first", [], [0xFFFFFFFF, 0], dict(family="G", unknown=True))]
    order = [by[f"G.A.L{L}.all"], plain[0], by["G.C.both_fields"], by["G.D.abc"], unknown[0], by["G.E.len3"], by[f"G.A.L{L}.last"], by[f"G.B.L{LB}.g255.mid"],
             plain[1], by["G.F.len16"], twice, by["G.F.order.yzx"], unknown[1], by["G.F.aba"], by["G.C.both_fields.or"], by["G.E.len2.or"]]
    rest = [q for q in queries if q.name not in {o.name for o in order}]
    return PhraseCase("G.batch", tb, d0, t0, order + rest, errors)


_BUILDERS = {}
for _L in A_LENGTHS:
    _BUILDERS[f"A.L{_L}"] = (lambda L=_L: _case_a(L))
for _L in B_LENGTHS:
    _BUILDERS[f"B.L{_L}"] = (lambda L=_L: _case_b(L))
_BUILDERS["C.title_only"] = lambda: _case_c("title_only")
_BUILDERS["C.both_fields"] = lambda: _case_c("both_fields")
_BUILDERS["D.mixing"] = lambda: _case_small("D.mixing", emit_field_mixing)
_BUILDERS["E.positions"] = lambda: _case_small("E.positions", emit_positions)
_BUILDERS["F.lengths"] = lambda: _case_small("F.lengths", emit_lengths)
_BUILDERS["G.batch"] = _case_g

CASE_NAMES = tuple(_BUILDERS)
FAMILIES = "ABCDEFG"
_CACHE = {}


def get_case(name):
    """The case of that name (built once per process)."""
    if name not in _CACHE:
        _CACHE[name] = _BUILDERS[name]()
    return _CACHE[name]


def pack(lists):
    """-> (ptr uint32 [n + 1], terms uint32) of a list of term lists."""
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint32)
    return ptr, np.array([t for x in lists for t in x], dtype=np.uint32)
