// facet_plan_harness.cpp — drives spaghettisearch_amd/csrc/facet_plan.hpp on the host (tests/test_facet_cpu.py compiles it with
// -fsanitize=address,undefined).  One command per line of stdin, one line of answer each:
//   g n_docs                               -> "words blocks last_block_words last_word_mask(hex) sum_block_words past_end_words past_end_mask(hex)"
//   l n_blocks n_active                    -> "n_launches covered max_grid first:count ..."  (covered: 1 if the launches hold every
//                                             block exactly once, in order)
//   a n_q has_q_ptr has_n_match n_buckets has_buckets has_bucket_out n_fields -> the check's code (0 OK, 1 INVALID, 2 UNSUPPORTED, 3 STATE)
//   f n_fields n_b field ...               -> the code of check_buckets over n_b buckets with these fields
//   b n_b {field lo hi} x n_b n_v {field value} x n_v
//                                          -> "n_cuts field_mask | lo_idx:hi_end x n_b | per value: its interval (-1: none) and the
//                                             buckets of its field that the table says hold it, as a hex mask"
// A last line "ok <n> lines" is printed at end of input.
#include "facet_plan.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>

namespace fp = ss::facetp;

int main() {
    char line[16384];
    long n_lines = 0;
    while (std::fgets(line, sizeof(line), stdin)) {
        std::istringstream in(line + 1);
        long long a = 0, b = 0, c = 0, d = 0, e = 0, f = 0, g = 0;
        if (line[0] == 'g' && (in >> a)) {
            const uint64_t n_docs = (uint64_t)a;
            const uint32_t nb = fp::blocks(n_docs);
            uint64_t sum = 0;
            for (uint32_t blk = 0; blk < nb; blk++) sum += fp::block_words(blk, n_docs);
            const uint64_t nw = fp::words(n_docs);
            std::printf("%" PRIu64 " %u %u %08x %" PRIu64 " %u %08x\n", nw, nb, nb ? fp::block_words(nb - 1, n_docs) : 0u,
                        nw ? fp::word_valid(nw - 1, n_docs) : 0u, sum, fp::block_words(nb, n_docs), fp::word_valid(nw, n_docs));
        } else if (line[0] == 'l' && (in >> a >> b)) {
            const std::vector<fp::Launch> ls = fp::launches((uint32_t)a, (uint32_t)b);
            uint64_t next = 0, max_grid = 0;
            bool covered = true;
            for (const fp::Launch& l : ls) {
                covered = covered && l.first == next && l.count >= 1;
                next += l.count;
                max_grid = std::max<uint64_t>(max_grid, (uint64_t)l.count * (uint64_t)b);
            }
            covered = covered && (b == 0 || next == (uint64_t)a);
            std::printf("%zu %d %" PRIu64, ls.size(), covered ? 1 : 0, max_grid);
            for (size_t i = 0; i < ls.size() && i < 4; i++) std::printf(" %u:%u", ls[i].first, ls[i].count);
            std::printf("\n");
        } else if (line[0] == 'a' && (in >> a >> b >> c >> d >> e >> f >> g)) {
            char msg[256] = "";
            const int rc = fp::check_args(msg, sizeof(msg), "harness", (int32_t)a, b != 0, c != 0, (int32_t)d, e != 0, f != 0, (int32_t)g);
            if ((rc != fp::OK) != (std::strlen(msg) > 0)) return 3;                // a refusal, and only a refusal, has a text
            std::printf("%d\n", rc);
        } else if (line[0] == 'f' && (in >> a >> b)) {
            std::vector<fp::Range> bk((size_t)b);
            for (auto& r : bk) { in >> c; r = fp::Range{(int32_t)c, 0, 0, 0}; }
            char msg[256] = "";
            const int rc = fp::check_buckets(msg, sizeof(msg), "harness", bk.data(), (int32_t)b, (int32_t)a);
            if ((rc != fp::OK) != (std::strlen(msg) > 0)) return 3;
            std::printf("%d\n", rc);
        } else if (line[0] == 'b' && (in >> a)) {
            std::vector<fp::Range> bk((size_t)a);
            for (auto& r : bk) {
                long long fld = 0, lo = 0, hi = 0;
                in >> fld >> lo >> hi;
                r = fp::Range{(int32_t)fld, 0, (int64_t)lo, (int64_t)hi};
            }
            fp::BucketTable t;
            fp::build_bucket_table(bk.data(), (int32_t)a, t);
            std::printf("%u %x |", t.n_cuts, t.field_mask);
            for (long long i = 0; i < a; i++) std::printf(" %u:%u", t.lo_idx[i], t.hi_end[i]);
            std::printf(" |");
            long long n_v = 0;
            in >> n_v;
            for (long long i = 0; i < n_v; i++) {
                long long fld = 0, v = 0;
                in >> fld >> v;
                const uint32_t iv = fp::interval_of(t.cuts, t.field_begin[fld], t.field_begin[fld + 1], (int64_t)v);
                uint64_t in_buckets = 0;
                for (long long k = 0; k < a; k++)
                    if (bk[k].field == fld && iv != fp::NO_INTERVAL && t.lo_idx[k] <= iv && iv < t.hi_end[k]) in_buckets |= 1ull << k;
                std::printf(" %lld:%" PRIx64, iv == fp::NO_INTERVAL ? -1ll : (long long)iv, in_buckets);
            }
            std::printf("\n");
        } else {
            std::fprintf(stderr, "bad line: %s", line);
            return 2;
        }
        n_lines++;
    }
    std::printf("ok %ld lines\n", n_lines);
    return 0;
}
