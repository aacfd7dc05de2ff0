// tstats_driver — csrc/tstats.cpp (bt_trade_stats_host, bt_tstats_agg_host, bt_tstats_merge, the
// argument rules) as a stand-alone host program, built with -fsanitize=address,undefined by
// test_tradestats_cpu.py.
//
//   tstats_driver IN OUT
// IN:  int32 S, P; then per lane, row-major: int32 n_trades, n_bars; n_trades bt_trade; n_bars int64
// OUT: S*P bt_tstats; P bt_tstats_agg of all rows; P bt_tstats_agg merged from the aggregates of
//      rows [0, S/2) and [S/2, S) (S >= 2; else the first again)
// stdout: one "refused: <message>" line per refusal tried, one "rule: <message>" line per rule.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "tstats.h"

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
    int32_t hdr[2];
    if (!rd(f, hdr, 2)) return 2;
    const int32_t S = hdr[0], P = hdr[1];
    // exactly sized buffers: a read past a lane's trades or bars is a heap overflow
    std::vector<bt_tstats> recs((size_t)S * P);
    for (size_t i = 0; i < recs.size(); ++i) {
        int32_t lane[2];
        if (!rd(f, lane, 2)) return 2;
        std::vector<bt_trade> trades((size_t)lane[0]);
        std::vector<int64_t> equity((size_t)lane[1]);
        if (!rd(f, trades.data(), trades.size()) || !rd(f, equity.data(), equity.size())) return 2;
        if (bt_trade_stats_host(lane[0], lane[0] ? trades.data() : nullptr, lane[1], equity.data(), &recs[i]) != 0) {
            fprintf(stderr, "%s\n", g_err.c_str());
            return 3;
        }
    }
    fclose(f);

    std::vector<bt_tstats_agg> whole((size_t)P), parts((size_t)2 * P), merged((size_t)P);
    if (bt_tstats_agg_host(S, P, recs.data(), whole.data()) != 0) return 3;
    if (S >= 2) {
        const int32_t h = S / 2;
        if (bt_tstats_agg_host(h, P, recs.data(), parts.data()) != 0) return 3;
        if (bt_tstats_agg_host(S - h, P, recs.data() + (size_t)h * P, parts.data() + P) != 0) return 3;
        if (bt_tstats_merge(parts.data(), 2, P, merged.data()) != 0) return 3;
    } else {
        if (bt_tstats_merge(whole.data(), 1, P, merged.data()) != 0) return 3;
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
    bt_tstats one;
    bt_tstats_agg a1;
    const int64_t eq[3] = {0, 5, -2};
    bt_trade t{0, 2, 1, 0, 100, 98};
    refused(bt_trade_stats_host(-1, &t, 3, eq, &one));
    refused(bt_trade_stats_host(1, &t, 0, eq, &one));
    refused(bt_trade_stats_host(1, &t, 3, eq, nullptr));
    refused(bt_trade_stats_host(1, &t, 3, nullptr, &one));
    refused(bt_trade_stats_host(1, nullptr, 3, eq, &one));
    refused(bt_trade_stats_host(1, &t, 2, eq, &one));
    t.side = 0;
    refused(bt_trade_stats_host(1, &t, 3, eq, &one));
    refused(bt_tstats_agg_host(-1, 1, &one, &a1));
    refused(bt_tstats_agg_host(1, 0, &one, &a1));
    refused(bt_tstats_agg_host(1, 1, &one, nullptr));
    refused(bt_tstats_agg_host(1, 1, nullptr, &a1));
    refused(bt_tstats_merge(&a1, 0, 1, &a1));
    refused(bt_tstats_merge(&a1, 1, 0, &a1));
    refused(bt_tstats_merge(nullptr, 1, 1, &a1));
    for (const std::string& why : {bt::tstats_refusal(false, 0, false, true, false),
                                   bt::tstats_refusal(true, -1, true, true, false),
                                   bt::tstats_refusal(true, (int64_t)BT_TSTATS_MAX + 1, true, true, false),
                                   bt::tstats_refusal(true, 3, false, true, false),
                                   bt::tstats_refusal(true, 3, true, true, true),
                                   bt::tstats_refusal(true, 3, true, false, false),
                                   bt::tstats_refusal(true, 0, false, false, false),
                                   bt::tstats_refusal(true, 0, false, false, true),
                                   bt::tstats_refusal(true, 0, true, false, false),
                                   bt::tstats_refusal(true, BT_TSTATS_MAX, true, true, false),
                                   bt::tstats_budget_refusal(400, 1000)})
        printf("rule: %s\n", why.c_str());
    t.side = -1;
    if (bt_trade_stats_host(1, &t, 3, eq, &one) != 0 || one.n_win != 1 || one.gross_win != 2 || one.mdd != 7) return 5;
    printf("ok %d %d\n", S, P);
    return 0;
}
