// match_lists.hpp — the list table of the calls that form a query's match set M(q) on the device (ss_facet_counts: facet.hip;
// ss_field_topk: field_topk.hip): per query its distinct usable terms' non-empty posting lists, title and body.  One host function
// builds it for both, so the two calls cannot come to disagree about which docs a query matches.  Host code only, apart from the
// layout of an entry, which the kernels read.
#pragma once
#include "scorer.hpp"

#include <algorithm>

namespace ss {

struct __attribute__((aligned(16))) MatchList { uint64_t b; uint32_t len, field; };   // postings [b, b + len) of the title (field 1) or body (0) table
static_assert(sizeof(MatchList) == 16, "list table layout");

struct MatchLists {
    std::vector<uint32_t> aq;                   // the queries that have a list, ascending
    std::vector<uint32_t> lptr{0u};             // [aq.size() + 1] their lists in `lists`
    std::vector<MatchList> lists;
};

// qptr [nq + 1] and terms: host copies, already checked.  A repeated term counts once; ids >= n_terms have no list.  More than
// SS_MAX_QUERY_TERMS distinct usable terms in a query: SS_ERR_UNSUPPORTED under `entry`'s name, as the scoring calls refuse them.
inline int32_t build_match_lists(ss_scorer* s, const char* entry, const uint32_t* qptr, const uint32_t* terms, size_t nq, MatchLists* out) {
    const std::vector<uint64_t>& tp = s->title->h_term_ptr;
    const std::vector<uint64_t>& bp = s->body->h_term_ptr;
    std::vector<uint32_t> dterm;
    for (size_t q = 0; q < nq; q++) {
        dterm.clear();
        for (uint32_t i = qptr[q]; i < qptr[q + 1]; i++) {
            const uint32_t t = terms[i];
            if ((uint64_t)t >= s->n_terms || std::find(dterm.begin(), dterm.end(), t) != dterm.end()) continue;
            dterm.push_back(t);
        }
        if (dterm.size() > SS_MAX_QUERY_TERMS)
            return s->ctx->fail(SS_ERR_UNSUPPORTED, "%s: query %zu has more than %d distinct terms", entry, q, SS_MAX_QUERY_TERMS);
        const size_t before = out->lists.size();
        for (const uint32_t t : dterm)
            for (uint32_t field = 0; field < 2; field++) {
                const uint64_t* const pp = field ? tp.data() : bp.data();
                if (pp[t + 1] > pp[t]) out->lists.push_back(MatchList{pp[t], (uint32_t)(pp[t + 1] - pp[t]), field});   // (a list is shorter than 2^32: ss_index_create)
            }
        if (out->lists.size() > before) {
            out->aq.push_back((uint32_t)q);
            out->lptr.push_back((uint32_t)out->lists.size());
        }
    }
    return SS_OK;
}

}  // namespace ss
