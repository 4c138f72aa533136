// Stand-alone harness of the term lexicon's host-only part (spaghettisearch_amd/csrc/lexicon_plan.hpp): compiled with the host C++
// compiler and no device header on the include path (tests/test_lexicon_plan_cpu.py, with -fsanitize=address,undefined).  It reads
// words from stdin, one per line as hex (an empty line = the empty word), and prints the sort order, the grouped layout and the
// chunk ranges, each checked here against a restatement first; a failing check exits with status 1.
#include "lexicon_plan.hpp"

#include <cstdio>
#include <iostream>
#include <string>

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "lexicon_plan_harness: %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
    using namespace ss::lex;
    std::vector<std::string> words;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::string w;
        for (size_t i = 0; i + 1 < line.size(); i += 2) w.push_back((char)std::stoi(line.substr(i, 2), nullptr, 16));
        words.push_back(w);
    }
    const uint64_t n = words.size();
    std::vector<uint64_t> ptr(n + 1, 0);
    std::string bytes;
    for (uint64_t t = 0; t < n; t++) { bytes += words[t]; ptr[t + 1] = bytes.size(); }
    const uint8_t* b = reinterpret_cast<const uint8_t*>(bytes.data());
    // ---- pointer arrays
    REQUIRE(word_ptr_ok(ptr.data(), n));
    if (n >= 2 && ptr[n] > 0) {
        std::vector<uint64_t> bad(ptr);
        bad[0] = 1;
        REQUIRE(!word_ptr_ok(bad.data(), n));
        bad = ptr;
        bad[n - 1] = bad[n] + 1;
        REQUIRE(!word_ptr_ok(bad.data(), n));
    }
    const uint32_t up[4] = {5, 5, 9, 9}, down[4] = {0, 4, 3, 8};
    REQUIRE(call_ptr_ok(up, 3) && !call_ptr_ok(down, 3) && call_ptr_ok(down, 0));
    // ---- order: a permutation, every neighbour pair in order under std::string's compare on unsigned chars
    std::vector<uint32_t> order;
    build_order(n, ptr.data(), b, order);
    REQUIRE(order.size() == n);
    std::vector<bool> seen(n, false);
    for (uint32_t t : order) { REQUIRE(t < n && !seen[t]); seen[t] = true; }
    for (uint64_t i = 0; i + 1 < n; i++) {
        const std::basic_string<unsigned char> x(words[order[i]].begin(), words[order[i]].end()), y(words[order[i + 1]].begin(), words[order[i + 1]].end());
        REQUIRE(x < y || (x == y && order[i] < order[i + 1]));
    }
    std::printf("order");
    for (uint32_t t : order) std::printf(" %u", t);
    std::printf("\n");
    // ---- groups: every word of at most 64 bytes once, by (length, id), its bytes at the group's stride, zero padding
    Groups g;
    build_groups(n, ptr.data(), b, g);
    uint64_t short_words = 0;
    for (auto& w : words) short_words += w.size() <= MAX_WORD;
    REQUIRE(g.start[0] == 0 && g.start[N_GROUPS] == short_words && g.gterm.size() == short_words && g.gwords.size() == g.base[N_GROUPS]);
    for (uint32_t L = 0; L < N_GROUPS; L++) {
        REQUIRE(g.start[L] <= g.start[L + 1] && g.base[L + 1] == g.base[L] + (uint64_t)(g.start[L + 1] - g.start[L]) * stride_words(L));
        for (uint32_t i = g.start[L]; i < g.start[L + 1]; i++) {
            const uint32_t t = g.gterm[i];
            REQUIRE(t < n && words[t].size() == L && (i == g.start[L] || g.gterm[i - 1] < t));
            const uint8_t* at = reinterpret_cast<const uint8_t*>(g.gwords.data() + g.base[L] + (uint64_t)(i - g.start[L]) * stride_words(L));
            for (uint32_t x = 0; x < 4 * stride_words(L); x++) REQUIRE(at[x] == (x < L ? (uint8_t)words[t][x] : 0));
        }
    }
    std::printf("starts");
    for (uint32_t L = 0; L < N_STARTS; L++) std::printf(" %u", g.start[L]);
    std::printf("\n");
    // ---- ranges and chunks
    for (uint64_t len = 0; len <= MAX_WORD + 2; len++)
        for (uint32_t d = 0; d <= 3; d++) {
            uint32_t lo = 7, hi = 7;
            suggest_range(g.start, len, d, &lo, &hi);
            uint64_t want = 0;
            for (auto& w : words)
                want += len <= MAX_WORD && w.size() <= MAX_WORD && (w.size() > len ? w.size() - len : len - w.size()) <= d;
            REQUIRE(lo <= hi && hi - lo == want);
            for (uint32_t chunk : {1u, 3u, 64u, 1u << 20}) {
                const uint64_t c = n_chunks(lo, hi, chunk);
                REQUIRE(c * chunk >= hi - lo && (c == 0 || (c - 1) * chunk < hi - lo));
            }
        }
    std::printf("ok %llu words\n", (unsigned long long)n);
    return 0;
}
