// ddboot_driver — csrc/ddboot.cpp (bt_drawdown_boot_host, the argument rules), the window rule it
// takes from csrc/bootstrap.cpp and plan_ddboot (csrc/plan.cpp) as a stand-alone host program, built
// with -fsanitize=address,undefined by test_ddboot_cpu.py.
//
//   ddboot_driver IN OUT
// IN:  int32 n, stride, from_bar, to_bar, B, L, Q, R; uint64 seed; Q int32 alpha_ppm; R int64 limits;
//      n int32 n_bars; n * stride int64 equity
// OUT: n bt_dd_lane; n * Q int64 quantiles; n * R int64 reach counts; n * B int64 raw values
// stdout: one "refused: <message>" line per refusal tried, one "rule: <message>" line per rule, one
// "plan: ..." line per plan.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ddboot.h"
#include "plan.h"

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
    int32_t hdr[8];
    uint64_t seed;
    if (!rd(f, hdr, 8) || !rd(f, &seed, 1)) return 2;
    const int32_t n = hdr[0], stride = hdr[1], from = hdr[2], to = hdr[3], B = hdr[4], L = hdr[5], Q = hdr[6], R = hdr[7];
    if (n < 1 || stride < 0 || B < 1 || Q < 0 || Q > BT_DD_LEVELS_MAX || R < 0 || R > BT_DD_LIMITS_MAX) return 2;
    // exactly sized buffers: a read past the levels, the limits, the bar counts or a row is a heap overflow
    std::vector<int32_t> levels((size_t)Q), n_bars((size_t)n);
    std::vector<int64_t> limits((size_t)R), equity((size_t)n * stride);
    if (!rd(f, levels.data(), levels.size()) || !rd(f, limits.data(), limits.size()) || !rd(f, n_bars.data(), n_bars.size()) ||
        !rd(f, equity.data(), equity.size()))
        return 2;
    fclose(f);
    std::vector<bt_dd_lane> recs((size_t)n), recs2((size_t)n);
    std::vector<int64_t> q((size_t)n * Q), reach((size_t)n * R), raw((size_t)n * B), q2((size_t)n * Q);
    if (bt_drawdown_boot_host(n, equity.data(), n_bars.data(), stride, from, to, B, L, seed, Q, levels.data(), R,
                              limits.data(), recs.data(), q.data(), reach.data(), raw.data()) != 0) {
        fprintf(stderr, "%s\n", g_err.c_str());
        return 3;
    }
    // each output alone gives the same bytes
    if (bt_drawdown_boot_host(n, equity.data(), n_bars.data(), stride, from, to, B, L, seed, 0, nullptr, 0, nullptr,
                              recs2.data(), nullptr, nullptr, nullptr) != 0 ||
        (Q > 0 && bt_drawdown_boot_host(n, equity.data(), n_bars.data(), stride, from, to, B, L, seed, Q, levels.data(), 0,
                                        nullptr, nullptr, q2.data(), nullptr, nullptr) != 0))
        return 3;
    if (memcmp(recs.data(), recs2.data(), recs.size() * sizeof(bt_dd_lane)) || (Q > 0 && memcmp(q.data(), q2.data(), q.size() * 8)))
        return 5;
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    if (!wr(f, recs.data(), recs.size()) || !wr(f, q.data(), q.size()) || !wr(f, reach.data(), reach.size()) ||
        !wr(f, raw.data(), raw.size()))
        return 2;
    fclose(f);

    // refusals: each returns -1 with a message and leaves the library usable
    auto refused = [&](int32_t rc) {
        if (rc != -1) exit(4);
        printf("refused: %s\n", g_err.c_str());
    };
    const int64_t eq[3] = {0, 5, -2};
    const int64_t wild[3] = {0, 1LL << 31, 0};
    const int32_t nb[1] = {3}, nb_long[1] = {4}, lv[2] = {1, 500000}, lv_zero[2] = {1, 0}, lv_big[2] = {1000001, 5};
    const int64_t lm[2] = {0, 9}, lm_neg[2] = {4, -1};
    bt_dd_lane r1;
    int64_t q1[2], c1[2], w1[4];
    auto call = [&](int32_t n_, const int64_t* e, const int32_t* b, int32_t fr, int32_t t, int32_t B_, int32_t L_, int32_t Q_,
                    const int32_t* a, int32_t R_, const int64_t* l, bool outs = true) {
        return bt_drawdown_boot_host(n_, e, b, 3, fr, t, B_, L_, 1, Q_, a, R_, l, outs ? &r1 : nullptr, outs ? q1 : nullptr,
                                     outs ? c1 : nullptr, outs ? w1 : nullptr);
    };
    refused(call(0, eq, nb, 0, 0, 4, 2, 2, lv, 2, lm));
    refused(call(1, eq, nb, -1, 2, 4, 2, 2, lv, 2, lm));
    refused(call(1, eq, nb, 0, 0, 0, 2, 2, lv, 2, lm));
    refused(call(1, eq, nb, 0, 0, 65537, 2, 2, lv, 2, lm));
    refused(call(1, eq, nb, 0, 0, 4, 0, 2, lv, 2, lm));
    refused(call(1, eq, nb, 0, 0, 4, 2, 9, lv, 2, lm));
    refused(call(1, eq, nb, 0, 0, 4, 2, 2, lv, 9, lm));
    refused(call(1, eq, nb, 0, 0, 4, 2, 2, nullptr, 2, lm));
    refused(call(1, eq, nb, 0, 0, 4, 2, 2, lv_zero, 2, lm));
    refused(call(1, eq, nb, 0, 0, 4, 2, 2, lv_big, 2, lm));
    refused(call(1, eq, nb, 0, 0, 4, 2, 2, lv, 2, nullptr));
    refused(call(1, eq, nb, 0, 0, 4, 2, 2, lv, 2, lm_neg));
    refused(call(1, eq, nb, 0, 0, 4, 2, 2, lv, 2, lm, false));
    refused(call(1, nullptr, nb, 0, 0, 4, 2, 2, lv, 2, lm));
    refused(call(1, eq, nb_long, 0, 0, 4, 2, 2, lv, 2, lm));
    refused(call(1, eq, nb, 2, 2, 4, 2, 2, lv, 2, lm));
    refused(call(1, wild, nb, 0, 0, 4, 2, 2, lv, 2, lm));
    const bt::DdCall ok{true, true, false, false, 0, 0, 100, 10, 2, lv, 2, lm, true, true, true, false};
    auto with = [&](auto change) {
        bt::DdCall c = ok;
        change(c);
        return bt::dd_refusal(c);
    };
    for (const std::string& why :
         {with([](bt::DdCall& c) { c.have_engine = false; }), with([](bt::DdCall& c) { c.have_dataset = false; }),
          with([](bt::DdCall& c) { c.n = 3; }), with([](bt::DdCall& c) { c.have_lanes = true; }),
          with([](bt::DdCall& c) { c.have_lanes = true, c.n = (int64_t)BT_BOOT_MAX + 1; }),
          with([](bt::DdCall& c) { c.staged = true, c.n = 2; }), with([](bt::DdCall& c) { c.from_bar = -3; }),
          with([](bt::DdCall& c) { c.have_rec = c.have_q = c.have_reach = false; }),
          with([](bt::DdCall& c) { c.have_rec = false, c.Q = c.R = 0; }), with([](bt::DdCall& c) { c.have_raw = true; }),
          with([](bt::DdCall& c) { c.have_lanes = true, c.n = BT_BOOT_MAX, c.have_raw = true; }),
          bt::dd_budget_refusal(10496, 2000), bt::dd_budget_refusal(2000, 2000), bt::dd_row_refusal(4831, 154600, 154624),
          bt::dd_row_refusal(4832, 154632, 154624)})
        printf("rule: %s\n", why.c_str());
    printf("rank: %lld %lld %lld %lld\n", (long long)bt::dd_rank(1000, 1), (long long)bt::dd_rank(1000, 950000),
           (long long)bt::dd_rank(1000, 950001), (long long)bt::dd_rank(65536, 1000000));
    for (const int32_t T : {100, 4831, 4832, 1 << 22}) {
        const bt::DdPlan pl = bt::plan_ddboot(n, T, B, 1, Q, R, true, false, false, 256, 0, 0);
        printf("plan: %d %d %d %zu %zu\n", pl.row_mode, pl.per_chunk, pl.chunks, pl.lds_bytes, pl.staging_bytes);
    }
    // equity 0, 5, -2 is d = 0, 5, -7; with L >= T a resample is a rotation of the row, and each of the three falls by 7
    if (call(1, eq, nb, 0, 0, 4, 3, 2, lv, 2, lm) != 0 || r1.sum != -2 || r1.mdd != 7 || r1.max_star != 7 || r1.min_star != 7 ||
        r1.n_ge != 4 || r1.m1.lo != 28 || r1.m2.lo != 196 || q1[0] != 7 || q1[1] != 7 || c1[0] != 4 || c1[1] != 0 || w1[3] != 7)
        return 5;
    printf("ok %d %d %d %d\n", n, B, Q, R);
    return 0;
}
