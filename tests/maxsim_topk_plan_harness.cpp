// maxsim_topk_plan_harness.cpp — drives spaghettisearch_amd/csrc/maxsim_topk_plan.hpp on the host (tests/test_maxsim_topk_cpu.py compiles
// it with -fsanitize=address,undefined).  One command per line of stdin, one line of answer each:
//   b dim qt k n_q lds_limit             -> "ok qb cap lds_bytes" of block()
//   c n v0 .. vn                         -> "n_slices cut[0] .. cut[n_slices]" of build_cuts over the tok_ptr of n docs ("0" alone: no slice)
//   h n_slices n_q qb k opt cu           -> "ok too_large n_qblocks chunk_slices n_chunks part_keys" of chunks()
//   v opt n_q qb k cu n v0 .. vn         -> "n_chunks covered max_tokens": the chunks of that plan over the cut table of that tok_ptr,
//                                           walked as the kernel walks them; covered: 1 if every doc that has a token lies in exactly one
//                                           chunk, the docs in none are the token-less ones behind the last token, the chunks are
//                                           consecutive and every cut is a doc boundary inside the table; max_tokens: the most tokens
//                                           that START in one chunk
// A last line "ok <n> lines" is printed at end of input.
#include "maxsim_topk_plan.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace tp = ss::mtp;

// "n v0 .. vn" -> the n + 1 values; false on a short line
static bool read_ptr(const char* s, std::vector<uint64_t>* out) {
    char* end = nullptr;
    const unsigned long long n = std::strtoull(s, &end, 10);
    if (end == s) return false;
    out->clear();
    for (unsigned long long i = 0; i <= n; i++) {
        s = end;
        const unsigned long long v = std::strtoull(s, &end, 10);
        if (end == s) return false;
        out->push_back(v);
    }
    return true;
}

int main() {
    static char line[1 << 20];
    long n_lines = 0;
    std::vector<uint64_t> vals;
    while (std::fgets(line, sizeof(line), stdin)) {
        long long a = 0, b = 0, c = 0, d = 0, e = 0, f = 0;
        int used = 0;
        if (line[0] == 'b' && std::sscanf(line + 1, "%lld %lld %lld %lld %lld", &a, &b, &c, &d, &e) == 5) {
            const tp::Block bl = tp::block((uint32_t)a, (uint32_t)b, (uint32_t)c, (uint64_t)d, (uint32_t)e);
            if (bl.ok && (bl.lds_bytes > (uint32_t)e || bl.cap < (uint32_t)c + tp::INC || bl.lds_bytes != tp::lds_of(bl.qb, (uint32_t)b, (uint32_t)a, bl.cap)))
                return 3;
            std::printf("%d %u %u %u\n", bl.ok ? 1 : 0, bl.qb, bl.cap, bl.lds_bytes);
        } else if (line[0] == 'c' && read_ptr(line + 1, &vals)) {
            std::vector<uint32_t> cut;
            tp::build_cuts(vals.data(), vals.size() - 1, &cut);
            std::printf("%zu", cut.empty() ? (size_t)0 : cut.size() - 1);
            for (uint32_t v : cut) std::printf(" %u", v);
            std::printf("\n");
        } else if (line[0] == 'h' && std::sscanf(line + 1, "%lld %lld %lld %lld %lld %lld", &a, &b, &c, &d, &e, &f) == 6) {
            const tp::Chunks ch = tp::chunks((uint64_t)a, (uint64_t)b, (uint32_t)c, (uint32_t)d, (int64_t)e, (uint32_t)f);
            std::printf("%d %d %u %" PRIu64 " %u %" PRIu64 "\n", ch.ok ? 1 : 0, ch.too_large ? 1 : 0, ch.n_qblocks, ch.chunk_slices, ch.n_chunks,
                        ch.part_keys);
        } else if (line[0] == 'v' && std::sscanf(line + 1, "%lld %lld %lld %lld %lld%n", &a, &b, &c, &d, &e, &used) == 5 &&
                   read_ptr(line + 1 + used, &vals)) {
            const uint64_t n_docs = vals.size() - 1;
            std::vector<uint32_t> cut;
            tp::build_cuts(vals.data(), n_docs, &cut);
            const uint64_t n_slices = cut.empty() ? 0 : cut.size() - 1;
            const tp::Chunks ch = tp::chunks(n_slices, (uint64_t)b, (uint32_t)c, (uint32_t)d, (int64_t)a, (uint32_t)e);
            bool covered = ch.ok;
            uint64_t max_tokens = 0;
            std::vector<uint32_t> seen((size_t)n_docs, 0);
            uint64_t next = 0;
            for (uint32_t i = 0; covered && i < ch.n_chunks; i++) {
                const uint64_t s0 = tp::chunk_first_slice(ch, i), s1 = tp::chunk_end_slice(ch, i, n_slices);
                if (s0 >= n_slices || s1 <= s0 || s1 > n_slices) { covered = false; break; }
                const uint64_t d0 = cut[(size_t)s0], d1 = cut[(size_t)s1];
                if (d0 != next || d1 < d0 || d1 > n_docs) { covered = false; break; }
                for (uint64_t x = d0; x < d1; x++) seen[(size_t)x]++;
                if (d1 > d0 && vals[(size_t)d1] - vals[(size_t)d0] > max_tokens) max_tokens = vals[(size_t)d1] - vals[(size_t)d0];
                next = d1;
            }
            if (ch.n_chunks) covered = covered && vals[(size_t)next] == vals[(size_t)n_docs] && next > 0 && vals[(size_t)next - 1] < vals[(size_t)next];
            else covered = covered && vals[(size_t)n_docs] == 0;                      // no chunk only for a table without a token
            if (ch.n_chunks)
                for (uint64_t x = 0; x < n_docs; x++) covered = covered && seen[(size_t)x] == (x < next ? 1u : 0u);
            std::printf("%u %d %" PRIu64 "\n", ch.n_chunks, covered ? 1 : 0, max_tokens);
        } else {
            std::fprintf(stderr, "bad line: %.80s", line);
            return 2;
        }
        n_lines++;
    }
    std::printf("ok %ld lines\n", n_lines);
    return 0;
}
