"""What ss_index_apply_delta(_pos) is defined to do (include/spaghetti_rank.h), restated with dicts.

A table is rows[term] = {doc: (weight float32, positions tuple)}.  One delta: every posting of `del_docs` goes, then the single
postings (del_term[i], del_doc[i]) go (a pair that is not there is ignored), then the postings (add_term[i], add_doc[i], add_w[i])
arrive with positions add_pos[add_pos_ptr[i] : add_pos_ptr[i + 1]] (none when add_pos_ptr is None).  A refused delta leaves
everything as it was.  flatten() lays the rows out as the CSR the library reads back: terms ascending, docs ascending inside a term.

Magnitudes (when the table's are resident): mag2[doc] = float64 sum of float32(w * w) over the doc's postings in ascending term
order, mag = sqrt(mag2).  A delta recomputes them for the docs it names (del_docs, the docs of the pairs, the docs of the
additions) and leaves every other doc's alone.

Nothing here knows how the device does it: no chunks, no searches, no flags.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

SS_ERR_INVALID = 1
SS_ERR_STATE = 6

# reason -> the library's return code
REFUSALS = {
    "held": SS_ERR_STATE,                 # a scorer holds the table
    "add_pos_ptr_start": SS_ERR_INVALID,  # add_pos_ptr[0] != 0
    "add_pos_ptr_order": SS_ERR_INVALID,  # add_pos_ptr decreases somewhere
    "del_docs_range": SS_ERR_INVALID,     # a doc of del_docs >= n_docs
    "pair_range": SS_ERR_INVALID,         # a pair's term >= n_terms or doc >= n_docs
    "add_range": SS_ERR_INVALID,          # an addition's term >= n_terms or doc >= n_docs
    "add_twice": SS_ERR_INVALID,          # the same (term, doc) twice among the additions
    "add_exists": SS_ERR_INVALID,         # the posting exists and this delta does not delete it
}

_Delta = namedtuple("Delta", "del_docs del_term del_doc add_term add_doc add_w add_pos_ptr add_pos")


def Delta(del_docs=(), del_pairs=((), ()), add=((), (), ()), add_pos=None):
    u = lambda v: np.asarray(v, dtype=np.uint32).reshape(-1)
    pp, pv = (None, None) if add_pos is None else (np.asarray(add_pos[0], dtype=np.uint64).reshape(-1), np.asarray(add_pos[1], dtype=np.float32).reshape(-1))
    d = _Delta(u(del_docs), u(del_pairs[0]), u(del_pairs[1]), u(add[0]), u(add[1]), np.asarray(add[2], dtype=np.float32).reshape(-1), pp, pv)
    assert len(d.del_term) == len(d.del_doc) and len(d.add_term) == len(d.add_doc) == len(d.add_w)
    assert pp is None or len(pp) == len(d.add_term) + 1
    return d


class Refused(Exception):
    def __init__(self, reason):
        super().__init__(reason)
        self.reason = reason
        self.code = REFUSALS[reason]


def _sum_squares(ws):
    """float64 sum, in the order given, of the float32 products w * w"""
    s = np.float64(0.0)
    for w in ws:
        s = s + np.float64(np.float32(w) * np.float32(w))
    return s


class TableModel:
    def __init__(self, n_docs, term_ptr, post_doc, post_w, pos_ptr=None, pos=None, mag_valid=False):
        self.n_docs = int(n_docs)
        self.n_terms = len(term_ptr) - 1
        self.positional = pos_ptr is not None
        self.rows = [dict() for _ in range(self.n_terms)]
        for t in range(self.n_terms):
            for i in range(int(term_ptr[t]), int(term_ptr[t + 1])):
                p = tuple(np.asarray(pos[int(pos_ptr[i]):int(pos_ptr[i + 1])], dtype=np.float32).tolist()) if self.positional else ()
                assert int(post_doc[i]) not in self.rows[t] and int(post_doc[i]) < self.n_docs
                self.rows[t][int(post_doc[i])] = (np.float32(post_w[i]), p)
        self.mag_valid = bool(mag_valid)
        self.mag2 = np.zeros(self.n_docs, dtype=np.float64)
        self.mag = np.zeros(self.n_docs, dtype=np.float64)
        if self.mag_valid:
            self.mag2, self.mag = self.full_magnitudes()

    # ---------------------------------------------------------------- read-out
    def n_post(self):
        return sum(len(r) for r in self.rows)

    def flatten(self):
        """-> (term_ptr uint64[T+1], post_doc uint32[P], post_w float32[P], pos_ptr uint64[P+1], pos float32[])"""
        tp, pd, pw, pp, pv = [0], [], [], [0], []
        for row in self.rows:
            for d in sorted(row):
                w, p = row[d]
                pd.append(d)
                pw.append(w)
                pv.extend(p)
                pp.append(len(pv))
            tp.append(len(pd))
        return (np.array(tp, dtype=np.uint64), np.array(pd, dtype=np.uint32), np.array(pw, dtype=np.float32),
                np.array(pp, dtype=np.uint64), np.array(pv, dtype=np.float32))

    def doc_magnitude(self, d):
        m2 = _sum_squares(row[d][0] for row in self.rows if d in row)        # rows in ascending term order
        return m2, np.sqrt(m2)

    def full_magnitudes(self):
        """(mag2, mag) of every doc from the table as it stands"""
        per_doc = [[] for _ in range(self.n_docs)]
        for row in self.rows:
            for d, (w, _) in row.items():
                per_doc[d].append(w)
        mag2 = np.array([_sum_squares(ws) for ws in per_doc], dtype=np.float64)
        return mag2, np.sqrt(mag2)

    # ---------------------------------------------------------------- one delta
    def check(self, delta, held=False):
        """raise Refused where the header says the call fails; touch nothing"""
        if held:
            raise Refused("held")
        n_add = len(delta.add_term)
        if self.positional and delta.add_pos_ptr is not None and n_add:
            if int(delta.add_pos_ptr[0]) != 0:
                raise Refused("add_pos_ptr_start")
            if any(int(delta.add_pos_ptr[i + 1]) < int(delta.add_pos_ptr[i]) for i in range(n_add)):
                raise Refused("add_pos_ptr_order")
        if any(int(d) >= self.n_docs for d in delta.del_docs):
            raise Refused("del_docs_range")
        if any(int(t) >= self.n_terms or int(d) >= self.n_docs for t, d in zip(delta.del_term, delta.del_doc)):
            raise Refused("pair_range")
        if any(int(t) >= self.n_terms or int(d) >= self.n_docs for t, d in zip(delta.add_term, delta.add_doc)):
            raise Refused("add_range")
        adds = list(zip(delta.add_term.tolist(), delta.add_doc.tolist()))
        if len(set(adds)) != len(adds):
            raise Refused("add_twice")
        gone_docs = set(delta.del_docs.tolist())
        gone_pairs = set(zip(delta.del_term.tolist(), delta.del_doc.tolist()))
        for t, d in adds:
            if d in self.rows[t] and d not in gone_docs and (t, d) not in gone_pairs:
                raise Refused("add_exists")

    def apply(self, delta, held=False):
        self.check(delta, held)
        gone = set(delta.del_docs.tolist())
        for row in self.rows:
            for d in gone & row.keys():
                del row[d]
        for t, d in zip(delta.del_term.tolist(), delta.del_doc.tolist()):
            self.rows[t].pop(d, None)
        use_pos = self.positional and delta.add_pos_ptr is not None
        for i, (t, d) in enumerate(zip(delta.add_term.tolist(), delta.add_doc.tolist())):
            assert d not in self.rows[t]
            p = tuple(delta.add_pos[int(delta.add_pos_ptr[i]):int(delta.add_pos_ptr[i + 1])].tolist()) if use_pos else ()
            self.rows[t][d] = (np.float32(delta.add_w[i]), p)
        if self.mag_valid:
            for d in self.touched(delta):
                self.mag2[d], self.mag[d] = self.doc_magnitude(d)

    @staticmethod
    def touched(delta):
        return sorted(set(delta.del_docs.tolist()) | set(delta.del_doc.tolist()) | set(delta.add_doc.tolist()))
