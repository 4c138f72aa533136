"""A second, independent restatement of the reference's quoted-phrase search, in plain Python and numpy.

Written from the Go text alone (retrieval/phrase.go:11-170 getPhraseFromInverted / evalPhraseOccurrence / getPosTerm,
retrieval/util.go:162-203 sortFloat32 / intersect), not from oracle/ and not from the kernels: the C oracle's orc_phrase is
what every kernel-vs-truth comparison of phrases goes through, and this module is what tests/test_phrase_cases_cpu.py holds
orc_phrase against, bit for bit.

A stored row is listPos = [weight, pos, pos, ...] (float32).  Here a row is the pair (weight float32, positions): `positions`
is listPos[1:], a Python list of floats holding float32 values exactly.

    getPosTerm (:120-170)    per phrase term i: map doc -> (title row, body row), every position shifted in float32,
                             listPos[j] -= float32(i)
    :25-44                   rows grouped per doc under the term's index in the phrase
    evalPhraseOccurrence     a doc counts only with an entry for EVERY index (:63); per field the float32 weights are summed
                             in phrase order (:59,69,73,83,90) and the shifted position lists intersected (:70,74,84,91);
                             a field whose intersection is non-empty gives a record with that field's sum (:97-105)
    intersect (util.go:179)  nil if either side is nil; both sides sorted (through float64, :162-177), then a two-pointer
                             multiset merge; the result stays nil when nothing was appended

nil and empty: Go's `x[1:]` of a one-element row is an EMPTY non-nil slice, intersect of an empty slice is nil, and every test
the reference makes on the result is len() != 0, so None (nil) and [] are told apart here only where the Go text does so.
"""
from __future__ import annotations

import numpy as np

F32_0 = np.float32(0.0)


def intersect(a, b):
    """util.go:179-203.  a, b: lists of floats or None (nil) -> list or None."""
    if a is None or b is None:                   # :180-182
        return None
    a, b = sorted(a), sorted(b)                  # :187-188 (sort.Float64s of the float32 values: the same order)
    ret = None                                   # var ret []float32
    i = j = 0
    while i != len(a) and j != len(b):           # :191
        if a[i] == b[j]:
            if ret is None:
                ret = []
            ret.append(a[i])
            i += 1
            j += 1
        elif a[i] > b[j]:
            j += 1
        else:
            i += 1
    return ret


class PhraseModel:
    """The phrase search over one pair of tables.  title / body = (term_ptr, post_doc, post_w), *_pos = (pos_ptr [P + 1], pos)."""

    def __init__(self, title, body, title_pos, body_pos):
        self.n_terms = len(body[0]) - 1
        assert len(title[0]) - 1 == self.n_terms
        self.fields = []
        for (ptr, doc, w), (pp, pv) in ((title, title_pos), (body, body_pos)):
            self.fields.append((np.asarray(ptr).astype(np.int64), np.asarray(doc).astype(np.int64).tolist(),
                                np.asarray(w, dtype=np.float32), np.asarray(pp).astype(np.int64), np.asarray(pv, dtype=np.float32)))
        self._rows = {}

    def _field_rows(self, field, term, i):
        """One table's answer for a term (inv.Get / getInvTitle) with the positions shifted as getPosTerm does: doc -> row."""
        ptr, doc, w, pp, pv = self.fields[field]
        lo, hi = int(ptr[term]), int(ptr[term + 1])
        a, b = int(pp[lo]), int(pp[hi])
        shifted = (pv[a:b] - np.float32(i)).astype(np.float32)            # :145 / :157 listPos[j] -= float32(term.Pos)
        assert shifted.dtype == np.float32
        shifted = shifted.tolist()
        cut = (pp[lo:hi + 1] - a).tolist()
        return {doc[lo + j]: (w[lo + j], shifted[cut[j]:cut[j + 1]]) for j in range(hi - lo)}

    def term_rows(self, term, i):
        """getPosTerm for phrase term `term` at index i: doc -> (title row | None, body row | None).  A word the tables do not
        know (badger.ErrKeyNotFound) gives an empty map."""
        key = (int(term), int(i))
        if key not in self._rows:
            out = {}
            if key[0] < self.n_terms:
                body = self._field_rows(1, key[0], key[1])
                title = self._field_rows(0, key[0], key[1])
                for d, row in body.items():                                # :142-152
                    out[d] = (None, row)
                for d, row in title.items():                               # :154-163
                    out[d] = (row, out[d][1] if d in out else None)
            self._rows[key] = out
        return self._rows[key]

    def phrase(self, phrase_terms):
        """-> (docs ascending uint32, title_sum float32, body_sum float32, flags uint8: bit 0 title, bit 1 body); the sum of a field
        without a record is 0 (the shape of oracle.phrase)."""
        m = len(phrase_terms)
        per_term = [self.term_rows(t, i) for i, t in enumerate(phrase_terms)]
        # :25-44 group by doc; :63 a doc is evaluated only when it has an entry under every index 0 .. m-1.  The indices are
        # distinct keys, so "as many entries as phrase terms" is "present in every term's map".
        docs = set(per_term[0]) if m else set()
        for rows in per_term[1:]:
            docs &= rows.keys()
        out = []
        for d in sorted(docs):
            sum_body, sum_title = F32_0, F32_0                             # :59
            body_x = title_x = None                                        # :60
            t_row, b_row = per_term[0][d]
            if b_row is not None:                                          # :68-71
                sum_body = np.float32(sum_body + b_row[0])
                body_x = b_row[1]
            if t_row is not None:                                          # :72-75
                sum_title = np.float32(sum_title + t_row[0])
                title_x = t_row[1]
            for i in range(1, m):                                          # :77-93
                t_row, b_row = per_term[i][d]
                if b_row is None:
                    body_x = None
                else:
                    sum_body = np.float32(sum_body + b_row[0])
                    body_x = intersect(body_x, b_row[1])
                if t_row is None:
                    title_x = None
                else:
                    sum_title = np.float32(sum_title + t_row[0])
                    title_x = intersect(title_x, t_row[1])
            has_b, has_t = bool(body_x), bool(title_x)                     # len(...) != 0
            if has_b or has_t:                                             # :97-106
                out.append((d, sum_title if has_t else F32_0, sum_body if has_b else F32_0, (1 if has_t else 0) | (2 if has_b else 0)))
        return (np.array([r[0] for r in out], dtype=np.uint32), np.array([r[1] for r in out], dtype=np.float32),
                np.array([r[2] for r in out], dtype=np.float32), np.array([r[3] for r in out], dtype=np.uint8))


def phrase(title, body, title_pos, body_pos, phrase_terms):
    """One phrase over the given tables, the call shape of oracle.phrase."""
    return PhraseModel(title, body, title_pos, body_pos).phrase(list(phrase_terms))
