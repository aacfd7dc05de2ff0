// costs.cpp — the net-of-costs figures on the host (docs/costs_spec.md): the argument rules of
// bt_costs, bt_costs_host (one lane's C records from its trade list and its gross equity curve),
// bt_costs_agg_host (the per-(parameter, level) reduction) and bt_costs_merge. Written from the
// spec, trade by trade and bar by bar with the compiler's __int128 and an integer division for the
// proportional fee; it shares no code with k_costs.hip but the split of an int128 into its words
// (host_common.h), so that the two check each other. Plain C++: no HIP call, builds with any host
// compiler.
#include "costs.h"

#include <cstring>
#include <exception>
#include <vector>

namespace bt {

std::string cost_levels_refusal(int64_t C, const int32_t* levels) {
    if (C < 1 || C > BT_COST_LEVELS_MAX)
        return "C = " + std::to_string(C) + " outside [1, " + std::to_string(BT_COST_LEVELS_MAX) + "]";
    if (!levels) return "levels is NULL";
    for (int64_t j = 0; j < C; ++j) {
        const int64_t fixed = levels[2 * j], bps = levels[2 * j + 1];
        if (fixed < 0 || fixed > BT_COST_FIXED_MAX)
            return "level " + std::to_string(j) + ": fixed = " + std::to_string(fixed) + " outside [0, " +
                   std::to_string(BT_COST_FIXED_MAX) + "]";
        if (bps < 0 || bps > BT_COST_BPS_MAX)
            return "level " + std::to_string(j) + ": bps = " + std::to_string(bps) + " outside [0, " +
                   std::to_string(BT_COST_BPS_MAX) + "]";
    }
    return "";
}

std::string costs_refusal(bool have_dataset, int64_t C, const int32_t* levels, int64_t n, bool have_lanes,
                          bool have_out, bool have_agg) {
    if (!have_dataset) return "no dataset loaded";
    const std::string why = cost_levels_refusal(C, levels);
    if (!why.empty()) return why;
    if (n < 0 || n > BT_COSTS_MAX)
        return "n = " + std::to_string(n) + " outside [0, " + std::to_string(BT_COSTS_MAX) + "]";
    if (!have_lanes) {
        if (n != 0) return "n = " + std::to_string(n) + " with lanes == NULL (all-lanes mode takes n = 0)";
        if (!have_out && !have_agg) return "out and agg are both NULL";
        return "";
    }
    if (have_agg) return "agg given in list mode (n = " + std::to_string(n) + " lanes): it must be NULL";
    if (n > 0 && !have_out) return "out is required in list mode (n = " + std::to_string(n) + " lanes)";
    return "";
}

std::string costs_budget_refusal(int64_t P, int64_t C, int64_t budget) {
    return "P * C = " + std::to_string(P) + " * " + std::to_string(C) + " records of one row (" +
           std::to_string(P * C * (int64_t)sizeof(bt_cost_rec)) + " bytes) exceed the staging budget of " +
           std::to_string(budget) + " bytes";
}

}  // namespace bt

namespace {

using bt::i128;
using bt::refuse;
using bt::wide_split;

// fee_j(px) of the spec
int64_t fill_fee(int64_t px, int64_t fixed, int64_t bps) { return fixed + px * bps / 10000; }

}  // namespace

extern "C" {

int32_t bt_costs_host(int32_t n_trades, const bt_trade* trades, int32_t n_bars, const int64_t* equity, int32_t C,
                      const int32_t* levels, bt_cost_rec* out) {
    const char* fn = "bt_costs_host";
    try {
        if (n_trades < 0) return refuse(fn, "n_trades = " + std::to_string(n_trades) + " is negative");
        if (n_bars < 1) return refuse(fn, "n_bars = " + std::to_string(n_bars) + " is below 1");
        const std::string why = bt::cost_levels_refusal(C, levels);
        if (!why.empty()) return refuse(fn, why);
        if (!out) return refuse(fn, "out is NULL");
        if (!equity) return refuse(fn, "equity is NULL");
        if (n_trades > 0 && !trades) return refuse(fn, "trades is NULL with n_trades = " + std::to_string(n_trades));
        for (int32_t i = 0; i < n_trades; ++i) {
            const bt_trade& t = trades[i];
            if (t.entry_bar < 0 || t.exit_bar < t.entry_bar || t.exit_bar >= n_bars)
                return refuse(fn, "trade " + std::to_string(i) + " runs [" + std::to_string(t.entry_bar) + ", " +
                                      std::to_string(t.exit_bar) + "] outside the " + std::to_string(n_bars) + " bars");
            if (t.side != 1 && t.side != -1)
                return refuse(fn, "trade " + std::to_string(i) + " has side " + std::to_string(t.side));
            if (t.entry_px < 0 || t.entry_px >= (1LL << 32) || t.exit_px < 0 || t.exit_px >= (1LL << 32))
                return refuse(fn, "trade " + std::to_string(i) + " fills at " + std::to_string(t.entry_px) + " and " +
                                      std::to_string(t.exit_px) + ", outside [0, 2^32)");
        }
        std::vector<int64_t> fee((size_t)n_bars);
        for (int32_t j = 0; j < C; ++j) {
            const int64_t fixed = levels[2 * j], bps = levels[2 * j + 1];
            bt_cost_rec r;
            memset(&r, 0, sizeof r);
            r.n_trades = n_trades;
            r.n_bars = n_bars;
            std::fill(fee.begin(), fee.end(), 0);
            for (int32_t i = 0; i < n_trades; ++i) {
                const bt_trade& t = trades[i];
                const int64_t fe = fill_fee(t.entry_px, fixed, bps), fx = fill_fee(t.exit_px, fixed, bps);
                fee[(size_t)t.entry_bar] += fe;
                fee[(size_t)t.exit_bar] += fx;
                r.turnover += t.entry_px + t.exit_px;
                const int64_t net = (int64_t)t.side * (t.exit_px - t.entry_px) - fe - fx;
                if (net > 0) r.n_win += 1, r.win_sum += net;
                else if (net < 0) r.n_loss += 1, r.loss_sum += -net;
            }
            int64_t paid = 0, peak = 0, before = 0;   // before: N_(t-1), N_(-1) = 0
            i128 s2 = 0;
            r.mdd_bar = -1;
            for (int32_t t = 0; t < n_bars; ++t) {
                paid += fee[(size_t)t];
                const int64_t N = equity[t] - paid;
                const int64_t step = N - before;
                s2 += (i128)step * (i128)step;
                before = N;
                if (N > peak) peak = N;
                const int64_t dd = peak - N;
                if (dd > r.mdd) r.mdd = dd, r.mdd_bar = t;
                if (dd > 0) r.underwater_bars += 1;
            }
            r.pnl = before;
            r.fees = paid;
            wide_split(s2, r.s2_lo, r.s2_hi);
            out[j] = r;
        }
        return 0;
    } catch (const std::exception& x) {
        return refuse(fn, std::string("exception: ") + x.what());
    }
}

int32_t bt_costs_agg_host(int32_t S, int32_t P, int32_t C, const bt_cost_rec* recs, bt_cost_agg* agg) {
    const char* fn = "bt_costs_agg_host";
    try {
        if (S < 0) return refuse(fn, "S = " + std::to_string(S) + " is negative");
        if (P < 1) return refuse(fn, "P = " + std::to_string(P) + " is below 1");
        if (C < 1 || C > BT_COST_LEVELS_MAX)
            return refuse(fn, "C = " + std::to_string(C) + " outside [1, " + std::to_string(BT_COST_LEVELS_MAX) + "]");
        if (!agg) return refuse(fn, "agg is NULL");
        if (S > 0 && !recs) return refuse(fn, "recs is NULL with S = " + std::to_string(S));
        const size_t PC = (size_t)P * (size_t)C;
        for (size_t q = 0; q < PC; ++q) {
            bt_cost_agg a;
            memset(&a, 0, sizeof a);
            for (int32_t s = 0; s < S; ++s) {
                const bt_cost_rec& r = recs[(size_t)s * PC + q];
                a.n_sym += 1;
                a.n_traded += r.n_trades > 0 ? 1 : 0;
                a.n_profit += r.pnl > 0 ? 1 : 0;
                a.trades += r.n_trades;
                a.pnl += r.pnl;
                a.fees += r.fees;
                if (r.mdd > a.mdd_max) a.mdd_max = r.mdd;
            }
            agg[q] = a;
        }
        return 0;
    } catch (const std::exception& x) {
        return refuse(fn, std::string("exception: ") + x.what());
    }
}

int32_t bt_costs_merge(const bt_cost_agg* in, int32_t world, int32_t PC, bt_cost_agg* out) {
    const char* fn = "bt_costs_merge";
    try {
        if (world < 1) return refuse(fn, "world = " + std::to_string(world) + " is below 1");
        if (PC < 1) return refuse(fn, "PC = " + std::to_string(PC) + " is below 1");
        if (!in || !out) return refuse(fn, "in and out are required");
        for (int32_t q = 0; q < PC; ++q) {
            bt_cost_agg a = in[q];
            for (int32_t w = 1; w < world; ++w) {
                const bt_cost_agg& b = in[(size_t)w * (size_t)PC + (size_t)q];
                a.n_sym += b.n_sym;
                a.n_traded += b.n_traded;
                a.n_profit += b.n_profit;
                a.trades += b.trades;
                a.pnl += b.pnl;
                a.fees += b.fees;
                if (b.mdd_max > a.mdd_max) a.mdd_max = b.mdd_max;
            }
            out[q] = a;
        }
        return 0;
    } catch (const std::exception& x) {
        return refuse(fn, std::string("exception: ") + x.what());
    }
}

}  // extern "C"
