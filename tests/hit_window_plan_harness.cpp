// hit_window_plan_harness.cpp — spaghettisearch_amd/csrc/hit_window_plan.hpp on its own: compiled by tests/test_hit_window_plan_cpu.py
// with the host compiler, no device header on the include path, under AddressSanitizer + UBSan.  Checks the paging check, the overlap
// test, the search for a bad count and copy_written itself and prints one "ok" line per group.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "hit_window_plan.hpp"

using namespace ss::hitwin;

static void require(bool ok, const char* what) {
    if (!ok) {
        std::fprintf(stderr, "hit_window_plan_harness: %s\n", what);
        std::exit(1);
    }
}

constexpr int32_t MAX_TOPK = 1024;                        // SS_MAX_TOPK of include/spaghetti_rank.h (the test compares them)

static int32_t paging(int32_t n_q, int32_t k_in, int32_t k, int32_t first, bool with_extra, int32_t extra, std::string* text = nullptr) {
    char msg[256] = "";
    const int32_t rc = check_paging(msg, sizeof(msg), "ss_entry", "k_window", MAX_TOPK, n_q, k_in, k, first, with_extra ? "g" : nullptr, extra);
    require((rc == OK) == (msg[0] == 0), "a refusal has a text and an acceptance has none");
    if (rc != OK) require(std::strstr(msg, "ss_entry") && std::strstr(msg, rc == INVALID && n_q < 0 ? "n_q" : "k_window"), "the text names entry and argument");
    if (text) *text = msg;
    return rc;
}

static void test_paging() {
    const int32_t edge[] = {0, 1, MAX_TOPK, MAX_TOPK + 1};
    for (int32_t k_in : edge)
        for (int32_t k : edge)
            for (int32_t first : {-1, 0, 1, INT32_MAX})
                for (int32_t n_q : {-1, 0, 1})
                    for (int ex = 0; ex < 3; ex++) {      // no extra, extra = 0, extra = 1
                        const int32_t want = n_q < 0 || k_in < 1 || k < 1 || (ex == 1) || first < 0 ? INVALID
                                             : k_in > MAX_TOPK || k > MAX_TOPK                     ? UNSUPPORTED
                                                                                                    : OK;
                        require(paging(n_q, k_in, k, first, ex != 0, ex == 1 ? 0 : 1) == want, "check_paging: wrong class");
                    }
    // which refusal wins: n_q, then the >= 1 group, then SS_MAX_TOPK; the offending value is in the text
    std::string text;
    require(paging(-1, 0, MAX_TOPK + 1, -1, true, 0, &text) == INVALID && text.find("n_q < 0") != std::string::npos, "n_q < 0 wins");
    require(paging(1, MAX_TOPK + 1, 0, 0, false, 1, &text) == INVALID && text.find("k = 0") != std::string::npos, "k < 1 wins over SS_MAX_TOPK");
    require(paging(1, MAX_TOPK + 1, 1, 0, false, 1, &text) == UNSUPPORTED && text.find("1025") != std::string::npos, "the width's value");
    require(paging(1, 1, 1, -1, false, 1, &text) == INVALID && text.find("first = -1") != std::string::npos, "first = -1");
    require(paging(1, 1, 1, 0, true, 0, &text) == INVALID && text.find("g = 0") != std::string::npos, "the extra argument's value");
    std::printf("ok paging\n");
}

static void test_overlap() {
    constexpr size_t ROW = 40, IN_ROWS = 6, OUT_ROWS = 4;
    std::vector<unsigned char> buf(ROW * (IN_ROWS + OUT_ROWS + 1));
    unsigned char* const in = buf.data();
    const size_t in_bytes = ROW * IN_ROWS, out_bytes = ROW * OUT_ROWS;
    require(overlaps(in, in_bytes, in, out_bytes), "offset 0");
    require(overlaps(in, in_bytes, in + 1, out_bytes), "offset 1");
    require(overlaps(in, in_bytes, in + ROW, out_bytes), "offset one row");
    require(overlaps(in, in_bytes, in + in_bytes - 1, out_bytes), "the input's last byte");
    require(!overlaps(in, in_bytes, in + in_bytes, out_bytes), "an output at the input's end is apart from it");
    require(!overlaps(in + out_bytes, in_bytes, in, out_bytes), "an output that ends at the input's start is apart from it");
    require(overlaps(in + 1, in_bytes, in, out_bytes), "an output whose last bytes reach into the input");
    std::printf("ok overlap\n");
}

static void test_bad_count() {
    constexpr int32_t K_IN = 5;
    constexpr size_t N = 7;
    const std::vector<int32_t> good = {0, 5, 1, 4, 2, 3, 5};
    require(first_bad_count(good.data(), N, K_IN) == NONE, "all counts inside");
    require(first_bad_count(good.data(), 0, K_IN) == NONE, "no counts");
    for (int32_t bad : {-1, K_IN + 1, INT32_MIN})
        for (size_t at : {(size_t)0, N / 2, N - 1}) {
            std::vector<int32_t> c = good;
            c[at] = bad;
            require(first_bad_count(c.data(), N, K_IN) == at, "the bad count's index");
            c[N - 1] = bad;                               // (a second one behind it: the first is reported)
            require(first_bad_count(c.data(), N, K_IN) == at, "the FIRST bad count's index");
        }
    std::printf("ok bad_count\n");
}

// copy_written against a byte-by-byte model: every byte of dst is compared afterwards, written or not
static void test_copy_written() {
    constexpr size_t STRIDE = 5, N_Q = 9;
    const int32_t counts[N_Q] = {0, 1, (int32_t)STRIDE, -1, (int32_t)STRIDE + 1, INT32_MIN, INT32_MAX, 3, 1};
    int cases = 0;
    for (size_t elem : {(size_t)4, (size_t)8, (size_t)16, (size_t)40})
        for (size_t inner_stride : {(size_t)1, (size_t)3, STRIDE})
            for (int mode = 0; mode < 2; mode++) {        // 0: whole entries; 1: per-query inner widths 0 .. inner_stride (and beyond: clamped)
                std::vector<uint32_t> inner_ptr(N_Q + 1, 7);
                for (size_t q = 0; q < N_Q; q++) inner_ptr[q + 1] = inner_ptr[q] + (uint32_t)(q == 2 ? inner_stride : q == 4 ? inner_stride + 2 : q % (inner_stride + 1));
                const size_t bytes = N_Q * STRIDE * inner_stride * elem;
                std::vector<unsigned char> src(bytes), dst(bytes), want(bytes);
                for (size_t i = 0; i < bytes; i++) {
                    src[i] = (unsigned char)(i * 7 + 1);
                    dst[i] = want[i] = (unsigned char)(0xA5 ^ (i * 3));
                }
                for (size_t q = 0; q < N_Q; q++) {
                    const size_t cnt = counts[q] < 0 ? 0 : (size_t)counts[q] > STRIDE ? STRIDE : (size_t)counts[q];
                    size_t inner = inner_stride;
                    if (mode == 1 && inner_ptr[q + 1] - inner_ptr[q] < inner) inner = inner_ptr[q + 1] - inner_ptr[q];
                    for (size_t j = 0; j < cnt; j++)
                        for (size_t b = 0; b < inner * elem; b++) {
                            const size_t at = ((q * STRIDE + j) * inner_stride) * elem + b;
                            want[at] = src[at];
                        }
                }
                copy_written(dst.data(), src.data(), N_Q, STRIDE, elem, counts, inner_stride, mode ? inner_ptr.data() : nullptr);
                require(dst == want, "copy_written: a byte differs from the model");
                cases++;
            }
    // no query at all, and the default inner width
    std::vector<unsigned char> a(16, 1), b(16, 2);
    copy_written(a.data(), b.data(), 0, 4, 4, nullptr);
    require(a == std::vector<unsigned char>(16, 1), "n_q = 0 writes nothing");
    const int32_t one = 2;
    copy_written(a.data(), b.data(), 1, 4, 4, &one);
    for (size_t i = 0; i < 16; i++) require(a[i] == (i < 8 ? 2 : 1), "the default inner width is one element");
    std::printf("ok copy_written %d\n", cases);
}

int main() {
    test_paging();
    test_overlap();
    test_bad_count();
    test_copy_written();
    std::printf("max_topk %d\n", MAX_TOPK);
    return 0;
}
