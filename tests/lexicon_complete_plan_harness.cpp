// Stand-alone harness of the completions' plan arithmetic (spaghettisearch_amd/csrc/lexicon_plan.hpp: complete_parts, complete_part):
// compiled with the host C++ compiler and no device header on the include path (tests/test_lexicon_complete_plan_cpu.py, with
// -fsanitize=address,undefined).  It takes no input; a failing check exits with status 1.
#include "lexicon_plan.hpp"

#include <cstdio>

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "lexicon_complete_plan_harness: %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
    using namespace ss::lex;
    // ---- the parts tile [lb, ub) exactly once and in order, their lengths differ by at most one
    unsigned long long ranges = 0;
    for (uint32_t P : {1u, 2u, 7u, 256u}) {
        const uint64_t lens[] = {0, 1, (uint64_t)P - 1, P, (uint64_t)P + 1, 64, 65, 0xFFFFFFFFull};
        for (uint64_t len : lens)
            for (uint32_t lb : {0u, 1u, 5u, 0x80000000u, 0xFFFFFFFFu}) {
                if ((uint64_t)lb + len > 0xFFFFFFFFull) continue;     // positions are below 2^32
                const uint32_t ub = (uint32_t)(lb + len);
                uint32_t at = lb, shortest = 0xFFFFFFFFu, longest = 0;
                for (uint32_t part = 0; part < P; part++) {
                    uint32_t b = 7, e = 7;
                    complete_part(lb, ub, P, part, &b, &e);
                    REQUIRE(b == at && e >= b && e <= ub);
                    shortest = e - b < shortest ? e - b : shortest;
                    longest = e - b > longest ? e - b : longest;
                    at = e;
                }
                REQUIRE(at == ub && longest - shortest <= 1);
                ranges++;
            }
    }
    // ---- P: within 1 .. 256 whatever n_q is; the option forces it inside that range and is ignored outside
    for (uint64_t n_q : {1ull, 2ull, 16ull, 17ull, 1024ull, 4096ull, 4097ull, 1ull << 20, 1ull << 31}) {
        const uint32_t P = complete_parts(n_q, 0);
        REQUIRE(P >= 1 && P <= DEFAULT_COMPLETE_PARTS && DEFAULT_COMPLETE_PARTS <= MAX_COMPLETE_PARTS);
        REQUIRE(n_q * P <= COMPLETE_WAVES || P == 1);             // not more waves than the target unless every prefix has one
        REQUIRE(P == DEFAULT_COMPLETE_PARTS || (uint64_t)(P + 1) * n_q > COMPLETE_WAVES);   // ... and no fewer than it allows
        for (int64_t forced : {1ll, 2ll, 7ll, 256ll}) REQUIRE(complete_parts(n_q, forced) == (uint32_t)forced);
        for (int64_t forced : {0ll, -1ll, 257ll, 1ll << 40}) REQUIRE(complete_parts(n_q, forced) == P);
    }
    REQUIRE(complete_parts(1, 0) == 64 && complete_parts(1024, 0) == 4 && complete_parts(1ull << 20, 0) == 1 && complete_parts(0, 0) == 64);
    std::printf("ok %llu ranges\n", ranges);
    return 0;
}
