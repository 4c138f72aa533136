// vector_plan_harness.cpp — spaghettisearch_amd/csrc/vector_plan.hpp on its own: compiled by tests/test_vector_cpu.py with the host
// compiler, no device header on the include path, under AddressSanitizer + UBSan.  Reads lines "n_docs dim n_q k chunk_docs n_cu lds"
// and prints the plan; checks the properties k_vec_topk relies on itself: the chunks cover every doc exactly once, none is empty,
// the LDS image fits, and a query's list can take what one check interval appends.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vector_plan.hpp"

static void require(bool ok, const char* what) {
    if (!ok) {
        std::fprintf(stderr, "vector_plan_harness: %s\n", what);
        std::exit(1);
    }
}

int main() {
    using namespace ss::vec;
    unsigned long long n_docs, dim, n_q, k, n_cu, lds;
    long long chunk;
    int lines = 0;
    while (std::scanf("%llu %llu %llu %llu %lld %llu %llu", &n_docs, &dim, &n_q, &k, &chunk, &n_cu, &lds) == 7) {
        const Plan p = plan(n_docs, (uint32_t)dim, n_q, (uint32_t)k, chunk, (uint32_t)n_cu, (uint32_t)lds);
        if (p.ok) {
            require(p.q_block == 16 || p.q_block == 32 || p.q_block == 64, "query block");
            require((uint64_t)p.n_qblocks * p.q_block >= n_q && (n_q == 0 || ((uint64_t)p.n_qblocks - 1) * p.q_block < n_q), "query blocks do not cover the queries");
            require(p.chunk_docs >= TILE && p.chunk_docs % TILE == 0, "a chunk is not a multiple of the tile");
            if (chunk > 0) require(p.chunk_docs == (uint32_t)((chunk + TILE - 1) / TILE * TILE), "the option's chunk size is not honoured");
            require((p.n_chunks == 0) == (n_docs == 0), "no chunk only without docs");
            require(p.cap >= k + TILE && p.cap < 65536, "a list cannot take one 16-doc step of the workgroup");
            require(p.lds_bytes <= lds && p.lds_bytes == lds_of(p.q_block, p.row_stride, p.cap), "the LDS image does not fit");
            require(p.row_stride >= dim && p.row_stride % 16 == 0, "query rows");
            require(p.part_keys == n_q * (uint64_t)p.n_chunks * k, "partial keys");
            // every doc in exactly one chunk, no chunk empty: walked doc by doc while that is cheap
            uint64_t covered = 0;
            std::vector<unsigned char> seen(n_docs <= 100000 ? (size_t)n_docs : 0, 0);
            for (uint32_t c = 0; c < p.n_chunks; c++) {
                const uint64_t b = chunk_begin(p, c), e = chunk_end(p, c, n_docs);
                require(b < e && e <= n_docs, "an empty chunk, or one past the table");
                require(b == covered, "a gap or an overlap between chunks");
                for (uint64_t d = b; d < e && !seen.empty(); d++) {
                    require(!seen[(size_t)d], "a doc in two chunks");
                    seen[(size_t)d] = 1;
                }
                covered = e;
            }
            require(covered == n_docs, "docs outside every chunk");
            for (unsigned char s : seen) require(s == 1, "a doc in no chunk");
        }
        std::printf("%d %d %u %u %u %u %u %u %u %llu\n", p.ok ? 1 : 0, p.too_large ? 1 : 0, p.q_block, p.n_qblocks, p.chunk_docs, p.n_chunks, p.cap,
                    p.row_stride, p.lds_bytes, (unsigned long long)p.part_keys);
        lines++;
    }
    std::printf("ok %d lines\n", lines);
    return 0;
}
