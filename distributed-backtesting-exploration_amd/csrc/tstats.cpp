// tstats.cpp — the per-lane trade statistics on the host (docs/tradestats_spec.md): the argument
// rules of bt_trade_stats, bt_trade_stats_host (one lane's record from its trade list and equity
// curve), bt_tstats_agg_host (the per-parameter reduction) and bt_tstats_merge. Written from the
// spec with the compiler's __int128 and shares no code with k_tstats.hip but the split of an
// int128 into its words (host_common.h), so that the two check each other. Plain C++: no HIP call,
// builds with any host compiler.
#include "tstats.h"

#include <cstring>
#include <exception>

namespace bt {

std::string tstats_refusal(bool have_dataset, int64_t n, bool have_lanes, bool have_out, bool have_agg) {
    if (!have_dataset) return "no dataset loaded";
    if (n < 0 || n > BT_TSTATS_MAX)
        return "n = " + std::to_string(n) + " outside [0, " + std::to_string(BT_TSTATS_MAX) + "]";
    if (!have_lanes) {
        if (n != 0) return "n = " + std::to_string(n) + " with lanes == NULL (all-lanes mode takes n = 0)";
        if (!have_out && !have_agg) return "out and agg are both NULL";
        return "";
    }
    if (have_agg) return "agg given in list mode (n = " + std::to_string(n) + " lanes): it must be NULL";
    if (n > 0 && !have_out) return "out is required in list mode (n = " + std::to_string(n) + " lanes)";
    return "";
}

std::string tstats_budget_refusal(int64_t P, int64_t budget) {
    return "P = " + std::to_string(P) + " records of one row (" + std::to_string(P * (int64_t)sizeof(bt_tstats)) +
           " bytes) exceed the staging budget of " + std::to_string(budget) + " bytes";
}

}  // namespace bt

namespace {

using bt::i128;
using bt::refuse;
using bt::wide_join;
using bt::wide_split;

// The trade hash of docs/oracle_spec.md §4: one mixed word per trade, summed mod 2^64.
uint64_t trade_word(int32_t entry_bar, int32_t exit_bar, int32_t side) {
    const uint64_t w = (uint64_t)(uint32_t)entry_bar | (uint64_t)(uint32_t)exit_bar << 31 | (uint64_t)(side > 0) << 62;
    const uint64_t z = (w ^ (w >> 29)) * 0xBF58476D1CE4E5B9ULL;
    return z ^ (z >> 32);
}

template <class T>
void keep_max(T& a, T b) {
    if (b > a) a = b;
}

// agg += one row's record
void agg_add(bt_tstats_agg& a, const bt_tstats& r) {
    a.n_sym += 1;
    a.n_traded += r.n_trades > 0 ? 1 : 0;
    keep_max(a.max_win_streak, r.max_win_streak);
    keep_max(a.max_loss_streak, r.max_loss_streak);
    keep_max(a.hold_max, r.hold_max);
    keep_max(a.max_underwater, r.max_underwater);
    a.n_trades += r.n_trades;
    a.n_win += r.n_win;
    a.n_loss += r.n_loss;
    a.n_long += r.n_long;
    a.n_long_win += r.n_long_win;
    a.hold_sum += r.hold_sum;
    a.hold_win += r.hold_win;
    a.gross_win += r.gross_win;
    a.gross_loss += r.gross_loss;
    keep_max(a.max_win, r.max_win);
    keep_max(a.max_loss, r.max_loss);
    keep_max(a.mdd_max, r.mdd);
    wide_split(wide_join(a.sq_lo, a.sq_hi) + wide_join(r.sq_lo, r.sq_hi), a.sq_lo, a.sq_hi);
}

// a += b, two aggregates of disjoint row sets
void agg_merge(bt_tstats_agg& a, const bt_tstats_agg& b) {
    a.n_sym += b.n_sym;
    a.n_traded += b.n_traded;
    keep_max(a.max_win_streak, b.max_win_streak);
    keep_max(a.max_loss_streak, b.max_loss_streak);
    keep_max(a.hold_max, b.hold_max);
    keep_max(a.max_underwater, b.max_underwater);
    a.n_trades += b.n_trades;
    a.n_win += b.n_win;
    a.n_loss += b.n_loss;
    a.n_long += b.n_long;
    a.n_long_win += b.n_long_win;
    a.hold_sum += b.hold_sum;
    a.hold_win += b.hold_win;
    a.gross_win += b.gross_win;
    a.gross_loss += b.gross_loss;
    keep_max(a.max_win, b.max_win);
    keep_max(a.max_loss, b.max_loss);
    keep_max(a.mdd_max, b.mdd_max);
    wide_split(wide_join(a.sq_lo, a.sq_hi) + wide_join(b.sq_lo, b.sq_hi), a.sq_lo, a.sq_hi);
}

}  // namespace

extern "C" {

int32_t bt_trade_stats_host(int32_t n_trades, const bt_trade* trades, int32_t n_bars, const int64_t* equity,
                            bt_tstats* out) {
    const char* fn = "bt_trade_stats_host";
    try {
        if (n_trades < 0) return refuse(fn, "n_trades = " + std::to_string(n_trades) + " is negative");
        if (n_bars < 1) return refuse(fn, "n_bars = " + std::to_string(n_bars) + " is below 1");
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
        }
        bt_tstats r;
        memset(&r, 0, sizeof r);
        r.n_trades = n_trades;
        r.n_bars = n_bars;
        int32_t win_run = 0, loss_run = 0;
        i128 sq = 0;
        for (int32_t i = 0; i < n_trades; ++i) {
            const bt_trade& t = trades[i];
            const int64_t pnl = (int64_t)t.side * (t.exit_px - t.entry_px);
            const int32_t hold = t.exit_bar - t.entry_bar;
            r.hold_sum += hold;
            keep_max(r.hold_max, hold);
            r.n_long += t.side > 0 ? 1 : 0;
            sq += (i128)pnl * (i128)pnl;
            r.hash += trade_word(t.entry_bar, t.exit_bar, t.side);
            if (pnl > 0) {
                r.n_win += 1;
                r.n_long_win += t.side > 0 ? 1 : 0;
                r.hold_win += hold;
                r.gross_win += pnl;
                keep_max(r.max_win, pnl);
                loss_run = 0;
                keep_max(r.max_win_streak, ++win_run);
            } else if (pnl < 0) {
                r.n_loss += 1;
                r.gross_loss += -pnl;
                keep_max(r.max_loss, -pnl);
                win_run = 0;
                keep_max(r.max_loss_streak, ++loss_run);
            } else {
                win_run = loss_run = 0;
            }
        }
        wide_split(sq, r.sq_lo, r.sq_hi);
        // the drawdown and the time under water, bar by bar
        int64_t peak = 0;
        int32_t peak_at = 0, run = 0;   // the first bar that holds the running peak (E_0 = 0)
        r.mdd_bar = r.peak_bar = -1;
        for (int32_t t = 0; t < n_bars; ++t) {
            const int64_t E = equity[t];
            if (E > peak) peak = E, peak_at = t;
            const int64_t dd = peak - E;
            if (dd > r.mdd) r.mdd = dd, r.mdd_bar = t, r.peak_bar = peak_at;
            if (dd > 0) {
                r.underwater_bars += 1;
                keep_max(r.max_underwater, ++run);
            } else {
                run = 0;
            }
        }
        *out = r;
        return 0;
    } catch (const std::exception& x) {
        return refuse(fn, std::string("exception: ") + x.what());
    }
}

int32_t bt_tstats_agg_host(int32_t S, int32_t P, const bt_tstats* recs, bt_tstats_agg* agg) {
    const char* fn = "bt_tstats_agg_host";
    try {
        if (S < 0) return refuse(fn, "S = " + std::to_string(S) + " is negative");
        if (P < 1) return refuse(fn, "P = " + std::to_string(P) + " is below 1");
        if (!agg) return refuse(fn, "agg is NULL");
        if (S > 0 && !recs) return refuse(fn, "recs is NULL with S = " + std::to_string(S));
        for (int32_t p = 0; p < P; ++p) {
            bt_tstats_agg a;
            memset(&a, 0, sizeof a);
            for (int32_t s = 0; s < S; ++s) agg_add(a, recs[(size_t)s * (size_t)P + (size_t)p]);
            agg[p] = a;
        }
        return 0;
    } catch (const std::exception& x) {
        return refuse(fn, std::string("exception: ") + x.what());
    }
}

int32_t bt_tstats_merge(const bt_tstats_agg* in, int32_t world, int32_t P, bt_tstats_agg* out) {
    const char* fn = "bt_tstats_merge";
    try {
        if (world < 1) return refuse(fn, "world = " + std::to_string(world) + " is below 1");
        if (P < 1) return refuse(fn, "P = " + std::to_string(P) + " is below 1");
        if (!in || !out) return refuse(fn, "in and out are required");
        for (int32_t p = 0; p < P; ++p) {
            bt_tstats_agg a = in[p];
            for (int32_t w = 1; w < world; ++w) agg_merge(a, in[(size_t)w * (size_t)P + (size_t)p]);
            out[p] = a;
        }
        return 0;
    } catch (const std::exception& x) {
        return refuse(fn, std::string("exception: ") + x.what());
    }
}

}  // extern "C"
