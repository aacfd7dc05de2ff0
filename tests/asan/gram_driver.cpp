// gram_driver — csrc/covariance.cpp (bt_covariance_host and the argument rules of bt_covariance and
// bt_gram_of) and the GramPlan of csrc/plan.cpp as a stand-alone host program, built with
// -fsanitize=address,undefined by test_gram_cpu.py.
//
//   gram_driver IN OUT
// IN:  int32 n, stride, from_bar, to_bar; n int32 n_bars; n*stride int64 equity
// OUT: n*n bt_wide gram, n int64 sums, int32 T
// stdout: one "refused: <message>" line per refusal tried, one "rule: <message>" line per rule, one
// "plan: ..." line per layout walked.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "covariance.h"
#include "plan.h"

static std::string g_err;
void bt::set_last_error(const std::string& s) { g_err = s; }

template <class T>
static bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <class T>
static bool wr(FILE* f, const T* p, size_t n) { return n == 0 || fwrite(p, sizeof(T), n, f) == n; }

// every region of a plan inside its staging, in order, on 256-byte boundaries
static void walk_plan(int32_t n, int32_t T, int cus, int32_t split) {
    const bt::GramPlan pl = bt::plan_gram(n, T, cus, split);
    const size_t at[5] = {pl.o_lanes, pl.o_d, pl.o_partial, pl.o_gram, pl.o_sums};
    const size_t len[5] = {(size_t)n * sizeof(bt::ReplayLane), (size_t)n * (size_t)pl.pitch * 4,
                           (size_t)pl.chunks * (size_t)pl.tiles * 256 * sizeof(bt_wide),
                           (size_t)n * (size_t)n * sizeof(bt_wide), (size_t)n * 8};
    size_t end = 0;
    for (int k = 0; k < 5; ++k) {
        if (at[k] % 256 != 0 || at[k] < end) exit(6);
        end = at[k] + len[k];
    }
    if (end > pl.staging_bytes || pl.staging_bytes < 256) exit(6);
    // the chunks cover the pitch, none of them empty
    if ((int64_t)pl.chunks * pl.chunk_bars < pl.pitch || (int64_t)(pl.chunks - 1) * pl.chunk_bars >= pl.pitch) exit(7);
    printf("plan: %d %d %d %d -> %d chunks of %d, %zu bytes\n", n, T, cus, split, pl.chunks, pl.chunk_bars,
           pl.staging_bytes);
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[4];
    if (!rd(f, hdr, 4)) return 2;
    const int32_t n = hdr[0], stride = hdr[1], from = hdr[2], to = hdr[3];
    std::vector<int32_t> nb((size_t)n);
    std::vector<int64_t> eq((size_t)n * stride);
    if (!rd(f, nb.data(), nb.size()) || !rd(f, eq.data(), eq.size())) return 2;
    fclose(f);

    // exactly sized outputs: a write past the end is a heap overflow
    std::vector<bt_wide> gram((size_t)n * n);
    std::vector<int64_t> sums((size_t)n);
    int32_t T = -1;
    if (bt_covariance_host(n, eq.data(), nb.data(), stride, from, to, gram.data(), sums.data(), &T) != 0) return 3;
    // each output alone equals the full call's
    std::vector<bt_wide> g2((size_t)n * n);
    std::vector<int64_t> s2((size_t)n);
    int32_t T2 = -1;
    if (bt_covariance_host(n, eq.data(), nb.data(), stride, from, to, g2.data(), nullptr, nullptr) != 0 ||
        bt_covariance_host(n, eq.data(), nb.data(), stride, from, to, nullptr, s2.data(), nullptr) != 0 ||
        bt_covariance_host(n, eq.data(), nb.data(), stride, from, to, nullptr, nullptr, &T2) != 0 || T2 != T ||
        (n && (memcmp(g2.data(), gram.data(), g2.size() * sizeof(bt_wide)) != 0 ||
               memcmp(s2.data(), sums.data(), s2.size() * 8) != 0)))
        return 5;
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    if (!wr(f, gram.data(), gram.size()) || !wr(f, sums.data(), sums.size()) || !wr(f, &T, 1)) return 2;
    fclose(f);

    auto refused = [&](int32_t rc) {
        if (rc != -1) exit(4);
        printf("refused: %s\n", g_err.c_str());
    };
    const int64_t e1[2] = {0, 0};
    const int32_t one = 2, three = 3;
    bt_wide g1;
    refused(bt_covariance_host(-1, e1, &one, 2, 0, 2, &g1, nullptr, nullptr));
    refused(bt_covariance_host(BT_COV_MAX + 1, e1, &one, 2, 0, 2, &g1, nullptr, nullptr));
    refused(bt_covariance_host(1, e1, &one, 2, -3, 2, &g1, nullptr, nullptr));
    refused(bt_covariance_host(1, e1, &one, 2, 7, 6, &g1, nullptr, nullptr));
    refused(bt_covariance_host(1, e1, &one, 2, 0, 2, nullptr, nullptr, nullptr));
    refused(bt_covariance_host(1, nullptr, &one, 2, 0, 2, &g1, nullptr, nullptr));
    refused(bt_covariance_host(1, e1, &three, 2, 0, 2, &g1, nullptr, nullptr));
    refused(bt_covariance_host(1, e1, &one, -1, 0, 2, &g1, nullptr, nullptr));

    printf("rule: %s\n", bt::covariance_refusal(false, 1, true, 0, 1, true).c_str());
    printf("rule: %s\n", bt::covariance_refusal(true, 3, false, 0, 1, true).c_str());
    printf("rule: %s\n", bt::covariance_refusal(true, 0, false, 0, 0, true).c_str());
    int32_t Tw = -1;
    printf("rule: %s\n", bt::covariance_window(1, INT_MAX, (1 << 22) + 2, Tw).c_str());
    printf("rule: %s\n", bt::covariance_window(1, INT_MAX, (1 << 22) + 1, Tw).c_str());
    printf("window: %d\n", Tw);
    printf("rule: %s\n", bt::covariance_window(900, 2000, 64, Tw).c_str());
    printf("window: %d\n", Tw);
    const int32_t d[6] = {1, -2147483647, 3, 4, INT_MIN, 6};
    printf("rule: %s\n", bt::gram_of_refusal(-1, 3, true, true).c_str());
    printf("rule: %s\n", bt::gram_of_refusal(2, (1 << 22) + 1, true, true).c_str());
    printf("rule: %s\n", bt::gram_of_refusal(2, 3, false, true).c_str());
    printf("rule: %s\n", bt::gram_of_refusal(2, 3, true, false).c_str());
    printf("rule: %s\n", bt::gram_of_refusal(2, 0, false, true).c_str());
    printf("rule: %s\n", bt::gram_domain_refusal(2, 3, d).c_str());
    printf("rule: %s\n", bt::gram_domain_refusal(1, 4, d).c_str());
    const bt::GramPlan big = bt::plan_gram(2048, 1 << 22, 256, 0);
    printf("rule: %s\n", bt::gram_staging_refusal(big.staging_bytes, bt::kGramStagingMax, 2048, 1 << 22).c_str());
    printf("rule: %s\n", bt::gram_staging_refusal(bt::kGramStagingMax, bt::kGramStagingMax, 1, 1).c_str());

    const int32_t shapes[8][2] = {{0, 0}, {1, 1}, {17, 65}, {2048, 2520}, {64, 491400}, {2, 1 << 22}, {33, 1000}, {5, 0}};
    for (const auto& s : shapes)
        for (const int32_t split : {0, 1, 2, 7, 100000}) walk_plan(s[0], s[1], 256, split);
    printf("ok %d %d\n", n, T);
    return 0;
}
