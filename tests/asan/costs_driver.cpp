// costs_driver — csrc/costs.cpp (bt_costs_host, bt_costs_agg_host, bt_costs_merge, the argument
// rules) and plan_costs (csrc/plan.cpp) as a stand-alone host program, built with
// -fsanitize=address,undefined by test_costs_cpu.py.
//
//   costs_driver IN OUT
// IN:  int32 S, P, C; C pairs int32 (fixed, bps); then per lane, row-major: int32 n_trades, n_bars;
//      n_trades bt_trade; n_bars int64
// OUT: S*P*C bt_cost_rec; P*C bt_cost_agg of all rows; P*C bt_cost_agg merged from the aggregates
//      of rows [0, S/2) and [S/2, S) (S >= 2; else the first again)
// stdout: one "refused: <message>" line per refusal tried, one "rule: <message>" line per rule, one
// "plan: ..." line per plan.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "costs.h"
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
    int32_t hdr[3];
    if (!rd(f, hdr, 3)) return 2;
    const int32_t S = hdr[0], P = hdr[1], C = hdr[2];
    if (C < 1 || C > BT_COST_LEVELS_MAX) return 2;
    // exactly sized buffers: a read past the levels, a lane's trades or its bars is a heap overflow
    std::vector<int32_t> levels((size_t)2 * C);
    if (!rd(f, levels.data(), levels.size())) return 2;
    std::vector<bt_cost_rec> recs((size_t)S * P * C);
    for (size_t i = 0; i < (size_t)S * P; ++i) {
        int32_t lane[2];
        if (!rd(f, lane, 2)) return 2;
        std::vector<bt_trade> trades((size_t)lane[0]);
        std::vector<int64_t> equity((size_t)lane[1]);
        if (!rd(f, trades.data(), trades.size()) || !rd(f, equity.data(), equity.size())) return 2;
        std::vector<bt_cost_rec> one((size_t)C);
        if (bt_costs_host(lane[0], lane[0] ? trades.data() : nullptr, lane[1], equity.data(), C, levels.data(),
                          one.data()) != 0) {
            fprintf(stderr, "%s\n", g_err.c_str());
            return 3;
        }
        memcpy(&recs[i * C], one.data(), (size_t)C * sizeof(bt_cost_rec));
    }
    fclose(f);

    const size_t PC = (size_t)P * C;
    std::vector<bt_cost_agg> whole(PC), parts(2 * PC), merged(PC);
    if (bt_costs_agg_host(S, P, C, recs.data(), whole.data()) != 0) return 3;
    if (S >= 2) {
        const int32_t h = S / 2;
        if (bt_costs_agg_host(h, P, C, recs.data(), parts.data()) != 0) return 3;
        if (bt_costs_agg_host(S - h, P, C, recs.data() + (size_t)h * PC, parts.data() + PC) != 0) return 3;
        if (bt_costs_merge(parts.data(), 2, (int32_t)PC, merged.data()) != 0) return 3;
    } else {
        if (bt_costs_merge(whole.data(), 1, (int32_t)PC, merged.data()) != 0) return 3;
    }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    if (!wr(f, recs.data(), recs.size()) || !wr(f, whole.data(), whole.size()) || !wr(f, merged.data(), merged.size()))
        return 2;
    fclose(f);

    // refusals: each returns -1 with a message and leaves the library usable
    auto refused = [&](int32_t rc) {
        if (rc != -1) exit(4);
        printf("refused: %s\n", g_err.c_str());
    };
    bt_cost_rec one[2];
    bt_cost_agg a1;
    const int64_t eq[3] = {0, 5, -2};
    const int32_t lv[4] = {1, 0, 0, 5};
    bt_trade t{0, 2, 1, 0, 100, 98};
    refused(bt_costs_host(-1, &t, 3, eq, 2, lv, one));
    refused(bt_costs_host(1, &t, 0, eq, 2, lv, one));
    refused(bt_costs_host(1, &t, 3, eq, 0, lv, one));
    refused(bt_costs_host(1, &t, 3, eq, 17, lv, one));
    refused(bt_costs_host(1, &t, 3, eq, 2, nullptr, one));
    const int32_t bad_fixed[4] = {1, 0, (1 << 20) + 1, 5}, bad_bps[4] = {1, 1001, 0, 5}, neg[4] = {-1, 0, 0, -5},
                  neg_bps[4] = {0, 0, 0, -5};
    refused(bt_costs_host(1, &t, 3, eq, 2, bad_fixed, one));
    refused(bt_costs_host(1, &t, 3, eq, 2, bad_bps, one));
    refused(bt_costs_host(1, &t, 3, eq, 2, neg, one));
    refused(bt_costs_host(1, &t, 3, eq, 2, neg_bps, one));
    refused(bt_costs_host(1, &t, 3, eq, 2, lv, nullptr));
    refused(bt_costs_host(1, &t, 3, nullptr, 2, lv, one));
    refused(bt_costs_host(1, nullptr, 3, eq, 2, lv, one));
    refused(bt_costs_host(1, &t, 2, eq, 2, lv, one));
    t.side = 0;
    refused(bt_costs_host(1, &t, 3, eq, 2, lv, one));
    t.side = 1, t.exit_px = 1LL << 32;
    refused(bt_costs_host(1, &t, 3, eq, 2, lv, one));
    t.exit_px = 98;
    refused(bt_costs_agg_host(-1, 1, 1, one, &a1));
    refused(bt_costs_agg_host(1, 0, 1, one, &a1));
    refused(bt_costs_agg_host(1, 1, 0, one, &a1));
    refused(bt_costs_agg_host(1, 1, 1, one, nullptr));
    refused(bt_costs_agg_host(1, 1, 1, nullptr, &a1));
    refused(bt_costs_merge(&a1, 0, 1, &a1));
    refused(bt_costs_merge(&a1, 1, 0, &a1));
    refused(bt_costs_merge(nullptr, 1, 1, &a1));
    for (const std::string& why : {bt::costs_refusal(false, 2, lv, 0, false, true, false),
                                   bt::costs_refusal(true, 0, lv, -1, false, false, false),
                                   bt::costs_refusal(true, 17, lv, -1, false, false, false),
                                   bt::costs_refusal(true, 2, nullptr, -1, false, false, false),
                                   bt::costs_refusal(true, 2, bad_fixed, -1, false, false, false),
                                   bt::costs_refusal(true, 2, bad_bps, -1, false, false, false),
                                   bt::costs_refusal(true, 2, lv, -1, true, true, false),
                                   bt::costs_refusal(true, 2, lv, (int64_t)BT_COSTS_MAX + 1, true, true, false),
                                   bt::costs_refusal(true, 2, lv, 3, false, true, false),
                                   bt::costs_refusal(true, 2, lv, 3, true, true, true),
                                   bt::costs_refusal(true, 2, lv, 3, true, false, false),
                                   bt::costs_refusal(true, 2, lv, 0, false, false, false),
                                   bt::costs_refusal(true, 2, lv, 0, false, false, true),
                                   bt::costs_refusal(true, 2, lv, 0, true, false, false),
                                   bt::costs_refusal(true, 16, nullptr, 0, true, false, false),
                                   bt::costs_refusal(true, 2, lv, BT_COSTS_MAX, true, true, false),
                                   bt::costs_budget_refusal(400, 8, 1000)})
        printf("rule: %s\n", why.c_str());
    for (const int64_t budget : {(int64_t)0, (int64_t)P * C * 48 + 600 + (int64_t)P * C * 88, (int64_t)100}) {
        const bt::CostsPlan pl = bt::plan_costs(S, P, C, false, 256, budget);
        printf("plan: %d %d %d %zu\n", pl.per_chunk, pl.chunks, pl.agg_slices, pl.staging_bytes);
    }
    if (bt_costs_host(1, &t, 3, eq, 2, lv, one) != 0 || one[0].n_loss != 1 || one[0].fees != 2 || one[0].pnl != -4 ||
        one[0].mdd != 8 || one[1].pnl != -2)
        return 5;
    printf("ok %d %d %d\n", S, P, C);
    return 0;
}
