// tail_driver — csrc/tail.cpp (bt_tail_host, the argument rules) and plan_tail (csrc/plan.cpp) as a
// stand-alone host program, built with -fsanitize=address,undefined by test_tail_cpu.py.
//
//   tail_driver IN OUT
// IN:  int32 n, stride, from_bar, to_bar, mode, Q; Q int32 alpha_ppm; n int32 n_bars; n * stride
//      int64 equity; n * stride int8 pos
// OUT: n bt_tail_rec; n * Q bt_tail_q
// stdout: one "refused: <message>" line per refusal tried, one "rule: <message>" line per rule, one
// "plan: ..." line per plan.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "plan.h"
#include "tail.h"

static std::string g_err;
void bt::set_last_error(const std::string& s) { g_err = s; }

template <class T>
static bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <class T>
static bool wr(FILE* f, const T* p, size_t n) { return n == 0 || fwrite(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[6];
    if (!rd(f, hdr, 6)) return 2;
    const int32_t n = hdr[0], stride = hdr[1], from = hdr[2], to = hdr[3], mode = hdr[4], Q = hdr[5];
    if (n < 0 || stride < 0 || Q < 1 || Q > BT_TAIL_LEVELS_MAX) return 2;
    // exactly sized buffers: a read past the levels, the bar counts or a row is a heap overflow
    std::vector<int32_t> levels((size_t)Q), n_bars((size_t)n);
    std::vector<int64_t> equity((size_t)n * stride);
    std::vector<int8_t> pos((size_t)n * stride);
    if (!rd(f, levels.data(), levels.size()) || !rd(f, n_bars.data(), n_bars.size()) ||
        !rd(f, equity.data(), equity.size()) || !rd(f, pos.data(), pos.size()))
        return 2;
    fclose(f);
    std::vector<bt_tail_rec> recs((size_t)n);
    std::vector<bt_tail_q> qs((size_t)n * Q);
    if (bt_tail_host(n, equity.data(), pos.data(), n_bars.data(), stride, from, to, mode, Q, levels.data(), recs.data(),
                     qs.data()) != 0) {
        fprintf(stderr, "%s\n", g_err.c_str());
        return 3;
    }
    // each output alone gives the same bytes
    std::vector<bt_tail_rec> recs2((size_t)n);
    std::vector<bt_tail_q> qs2((size_t)n * Q);
    if (bt_tail_host(n, equity.data(), pos.data(), n_bars.data(), stride, from, to, mode, Q, levels.data(), recs2.data(),
                     nullptr) != 0 ||
        bt_tail_host(n, equity.data(), pos.data(), n_bars.data(), stride, from, to, mode, Q, levels.data(), nullptr,
                     qs2.data()) != 0)
        return 3;
    if ((n && memcmp(recs.data(), recs2.data(), recs.size() * sizeof(bt_tail_rec))) ||
        (n && memcmp(qs.data(), qs2.data(), qs.size() * sizeof(bt_tail_q))))
        return 5;
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    if (!wr(f, recs.data(), recs.size()) || !wr(f, qs.data(), qs.size())) return 2;
    fclose(f);

    // refusals: each returns -1 with a message and leaves the library usable
    auto refused = [&](int32_t rc) {
        if (rc != -1) exit(4);
        printf("refused: %s\n", g_err.c_str());
    };
    const int64_t eq[3] = {0, 5, -2};
    const int64_t wild[3] = {0, 1LL << 31, 0};
    const int8_t ps[3] = {1, 1, 0};
    const int32_t nb[1] = {3}, nb_long[1] = {4}, lv[2] = {1, 500000};
    const int32_t lv_zero[2] = {1, 0}, lv_big[2] = {1000001, 5};
    bt_tail_rec r1;
    bt_tail_q q2[2];
    refused(bt_tail_host(-1, eq, ps, nb, 3, 0, 0, 0, 2, lv, &r1, q2));
    refused(bt_tail_host(1, eq, ps, nb, 3, 0, 0, 0, 0, lv, &r1, q2));
    refused(bt_tail_host(1, eq, ps, nb, 3, 0, 0, 0, 9, lv, &r1, q2));
    refused(bt_tail_host(1, eq, ps, nb, 3, 0, 0, 0, 2, nullptr, &r1, q2));
    refused(bt_tail_host(1, eq, ps, nb, 3, 0, 0, 0, 2, lv_zero, &r1, q2));
    refused(bt_tail_host(1, eq, ps, nb, 3, 0, 0, 0, 2, lv_big, &r1, q2));
    refused(bt_tail_host(1, eq, ps, nb, 3, 0, 0, 2, 2, lv, &r1, q2));
    refused(bt_tail_host(1, eq, ps, nb, 3, -1, 2, 0, 2, lv, &r1, q2));
    refused(bt_tail_host(1, eq, ps, nb, 3, 2, 2, 0, 2, lv, &r1, q2));
    refused(bt_tail_host(1, eq, ps, nb, 3, 0, 0, 0, 2, lv, nullptr, nullptr));
    refused(bt_tail_host(1, nullptr, ps, nb, 3, 0, 0, 0, 2, lv, &r1, q2));
    refused(bt_tail_host(1, eq, ps, nb_long, 3, 0, 0, 0, 2, lv, &r1, q2));
    refused(bt_tail_host(1, eq, nullptr, nb, 3, 0, 0, 1, 2, lv, &r1, q2));
    refused(bt_tail_host(1, wild, ps, nb, 3, 0, 0, 0, 2, lv, &r1, q2));
    for (const std::string& why : {bt::tail_refusal(false, 0, false, 0, 0, 0, 2, lv, true, true, 100),
                                   bt::tail_refusal(true, 0, true, 0, 0, 0, 2, lv, true, true, 100),
                                   bt::tail_refusal(true, (int64_t)BT_TAIL_MAX + 1, true, 0, 0, 0, 2, lv, true, true, 100),
                                   bt::tail_refusal(true, 3, false, 0, 0, 0, 2, lv, true, true, 100),
                                   bt::tail_refusal(true, 0, false, 0, 0, 0, 0, lv, true, true, 100),
                                   bt::tail_refusal(true, 0, false, 0, 0, 0, 2, nullptr, true, true, 100),
                                   bt::tail_refusal(true, 0, false, 0, 0, 0, 2, lv_zero, true, true, 100),
                                   bt::tail_refusal(true, 0, false, 0, 0, 7, 2, lv, true, true, 100),
                                   bt::tail_refusal(true, 0, false, 5, 3, 0, 2, lv, true, true, 100),
                                   bt::tail_refusal(true, 0, false, 0, 0, 0, 2, lv, false, false, 100),
                                   bt::tail_refusal(true, 0, false, 0, 0, 0, 2, lv, true, false, (1 << 22) + 1),
                                   bt::tail_refusal(true, 0, false, 0, 0, 1, 2, lv, false, true, 1 << 22),
                                   bt::tail_refusal(true, BT_TAIL_MAX, true, 3, 9, 1, 2, lv, true, true, 100),
                                   bt::tail_of_refusal(0, 5, true, 2, lv, true, true),
                                   bt::tail_of_refusal(1, 0, true, 2, lv, true, true),
                                   bt::tail_of_refusal(1, (1 << 22) + 1, true, 2, lv, true, true),
                                   bt::tail_of_refusal(1, 5, false, 2, lv, true, true),
                                   bt::tail_of_refusal(1, 5, true, 9, lv, true, true),
                                   bt::tail_of_refusal(1, 5, true, 2, lv, false, false),
                                   bt::tail_of_refusal(BT_TAIL_MAX, 1 << 22, true, 2, lv, false, true),
                                   bt::tail_row_refusal(14081, 56324, 56320), bt::tail_budget_refusal(true, 6656, 2000),
                                   bt::tail_budget_refusal(false, 1600, 100)})
        printf("rule: %s\n", why.c_str());
    printf("longest: %d %d %d %d\n", bt::tail_longest(0, 0, 700), bt::tail_longest(10, 20, 700), bt::tail_longest(10, 900, 700),
           bt::tail_longest(700, 900, 700));
    for (const int32_t longest : {100, 14080, 14081, 1 << 22}) {
        const bt::TailPlan pl = bt::plan_tail(n > 0 ? n : 1, 1, Q, true, false, longest, 256, 0, 0);
        printf("plan: %d %d %d %zu %zu\n", pl.row_mode, pl.per_chunk, pl.chunks, pl.lds_bytes, pl.staging_bytes);
    }
    if (bt_tail_host(1, eq, ps, nb, 3, 0, 0, 0, 2, lv, &r1, q2) != 0 || r1.n != 3 || r1.s1 != -2 || r1.min_d != -7 ||
        r1.min_bar != 2 || r1.s4[0] != 625 + 2401 || q2[0].var != -7 || q2[1].k != 2 || q2[1].var != 0 || q2[1].es_sum != -7)
        return 5;
    printf("ok %d %d\n", n, Q);
    return 0;
}
