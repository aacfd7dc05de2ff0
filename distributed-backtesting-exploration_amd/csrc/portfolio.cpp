// portfolio.cpp — the host rules of bt_portfolio (portfolio.h) and the scalar restatement of what
// k_portfolio.hip computes: bt_portfolio_host, from per-entry curves as bt_replay returns them, and
// bt_portfolio_merge. Written from docs/portfolio_spec.md with the compiler's __int128; it shares
// only the Sharpe formula (internal.h sharpe_ticks) with the kernels, so that the two check each
// other. Pure code: no HIP call, no device state.
#include "portfolio.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <exception>

#include "replay.h"

namespace bt {

std::string portfolio_refusal(bool have_dataset, int64_t n, bool have_lanes, int64_t T, bool any_output) {
    if (!have_dataset) return "no dataset loaded";
    if (n < 0 || n > BT_PORTFOLIO_MAX)
        return "n = " + std::to_string(n) + " outside [0, " + std::to_string(BT_PORTFOLIO_MAX) + "]";
    if (n > 0 && !have_lanes) return "lanes are required";
    if (T < 1 || T > kPortfolioMaxT)
        return "T = " + std::to_string(T) + " outside [1, " + std::to_string(kPortfolioMaxT) + "]";
    if (!any_output) return "pnl, equity, n_long, n_short and summary are all NULL";
    return "";
}

std::string portfolio_window(int64_t i, int32_t from_bar, int32_t to_bar, int32_t bars, int32_t T,
                             int32_t& from, int32_t& to) {
    if (from_bar < 0)
        return "from_bar = " + std::to_string(from_bar) + " is negative (entry " + std::to_string(i) + ")";
    if (to_bar < from_bar)
        return "to_bar = " + std::to_string(to_bar) + " is below from_bar = " + std::to_string(from_bar) +
               " (entry " + std::to_string(i) + ")";
    from = from_bar;
    to = std::max(from_bar, std::min(to_bar, std::min(bars, T)));
    return "";
}

std::string PfResolved::count(int32_t from, int32_t to) {
    window_bars += to - from;
    if (window_bars > kPortfolioMaxWindowBars)
        return "the windows hold " + std::to_string(window_bars) + " bars or more, above 2^30";
    lo = n_lanes ? std::min(lo, from) : from;
    hi = n_lanes ? std::max(hi, to) : to;
    ++n_lanes;
    return "";
}

std::string portfolio_resolve(const SymDesc* syms, size_t n_sym, int32_t P, int32_t n, const bt_pf_lane* lanes,
                              int32_t T, PfResolved& out) {
    out = PfResolved{};
    out.req.reserve((size_t)std::max(n, 0));
    return resolve_lanes(syms, n_sym, P, n, lanes, "entry", [&](int32_t i, const LaneRef& ref) {
        int32_t from, to;
        std::string why = portfolio_window(i, lanes[i].from_bar, lanes[i].to_bar, ref.bars, T, from, to);
        if (!why.empty() || to <= from) return why;
        why = out.count(from, to);
        if (why.empty()) out.req.push_back(PfLane{ref, from, to});
        return why;
    });
}

void portfolio_finish_host(int32_t T, int32_t n_lanes, int32_t lo, int32_t hi, const int64_t* pnl,
                           const int32_t* n_long, const int32_t* n_short, double sqrt_ann, int64_t* equity,
                           bt_pf_summary* sum) {
    int64_t eq = 0, peak = 0, mdd = 0, expo = 0;
    int32_t gross = 0;
    i128 s1 = 0, s2 = 0;
    for (int32_t t = 0; t < T; ++t) {
        eq += pnl[t];
        if (equity) equity[t] = eq;
        peak = std::max(peak, eq);
        mdd = std::max(mdd, peak - eq);
        const int32_t g = n_long[t] + n_short[t];
        gross = std::max(gross, g);
        expo += g;
        if (t >= lo && t < hi) {
            s1 += (i128)pnl[t];
            s2 += (i128)pnl[t] * (i128)pnl[t];
        }
    }
    if (!sum) return;
    memset(sum, 0, sizeof *sum);
    sum->n_lanes = n_lanes;
    sum->first_bar = lo;
    sum->n_bars = hi - lo;
    sum->max_gross = gross;
    sum->pnl = eq;
    sum->mdd = mdd;
    sum->exposure = expo;
    wide_split(s1, sum->s1_lo, sum->s1_hi);
    wide_split(s2, sum->s2_lo, sum->s2_hi);
    sum->sharpe = sharpe_ticks(s1, s2, hi - lo, sqrt_ann);
}

}  // namespace bt

namespace {

using bt::refuse;

// The merged or restated rows into the caller's buffers (any may be NULL).
void give(int32_t T, const std::vector<int64_t>& pnl, const std::vector<int32_t>& nl, const std::vector<int32_t>& ns,
          int64_t* out_pnl, int32_t* out_long, int32_t* out_short) {
    if (out_pnl) memcpy(out_pnl, pnl.data(), (size_t)T * sizeof(int64_t));
    if (out_long) memcpy(out_long, nl.data(), (size_t)T * sizeof(int32_t));
    if (out_short) memcpy(out_short, ns.data(), (size_t)T * sizeof(int32_t));
}

}  // namespace

extern "C" {

int32_t bt_portfolio_host(int32_t n, const int64_t* equity, const int8_t* pos, const int32_t* n_bars,
                          int64_t stride, const bt_pf_lane* lanes, int32_t T, int64_t annualization,
                          int64_t* out_pnl, int64_t* out_equity, int32_t* out_long, int32_t* out_short,
                          bt_pf_summary* summary) {
    const char* fn = "bt_portfolio_host";
    try {
        const std::string why = bt::portfolio_refusal(true, n, lanes != nullptr, T,
                                                      out_pnl || out_equity || out_long || out_short || summary);
        if (!why.empty()) return refuse(fn, why);
        if (annualization <= 0)
            return refuse(fn, "annualization = " + std::to_string(annualization) + " is not positive");
        int32_t b_max = 0;
        const std::string c = bt::curves_refusal(n, equity && pos && n_bars, "equity, pos and n_bars", n_bars, stride,
                                                 "entry", b_max);
        if (!c.empty()) return refuse(fn, c);
        bt::PfResolved r;
        std::vector<int64_t> pnl((size_t)T, 0);
        std::vector<int32_t> nl((size_t)T, 0), ns((size_t)T, 0);
        for (int32_t i = 0; i < n; ++i) {
            int32_t from, to;
            std::string w = bt::portfolio_window(i, lanes[i].from_bar, lanes[i].to_bar, n_bars[i], T, from, to);
            if (!w.empty()) return refuse(fn, w);
            if (to <= from) continue;
            w = r.count(from, to);
            if (!w.empty()) return refuse(fn, w);
            const int64_t* E = equity + (size_t)i * (size_t)stride;
            const int8_t* ps = pos + (size_t)i * (size_t)stride;
            for (int32_t t = from; t < to; ++t) {
                pnl[t] += E[t] - (t > 0 ? E[t - 1] : 0);
                nl[t] += ps[t] > 0;
                ns[t] += ps[t] < 0;
            }
        }
        bt::portfolio_finish_host(T, r.n_lanes, r.lo, r.hi, pnl.data(), nl.data(), ns.data(),
                                  std::sqrt((double)annualization), out_equity, summary);
        give(T, pnl, nl, ns, out_pnl, out_long, out_short);
        return 0;
    } catch (const std::exception& x) {
        return refuse(fn, std::string("exception: ") + x.what());
    }
}

int32_t bt_portfolio_merge(int32_t world, int32_t T, const int64_t* pnl, const int32_t* n_long,
                           const int32_t* n_short, const bt_pf_summary* summaries, int64_t annualization,
                           int64_t* out_pnl, int64_t* out_equity, int32_t* out_long, int32_t* out_short,
                           bt_pf_summary* summary) {
    const char* fn = "bt_portfolio_merge";
    try {
        if (world < 1) return refuse(fn, "world = " + std::to_string(world) + " is below 1");
        if (T < 1 || T > bt::kPortfolioMaxT)
            return refuse(fn, "T = " + std::to_string(T) + " outside [1, " + std::to_string(bt::kPortfolioMaxT) + "]");
        if (!pnl || !n_long || !n_short || !summaries) return refuse(fn, "pnl, n_long, n_short and summaries are required");
        if (!(out_pnl || out_equity || out_long || out_short || summary))
            return refuse(fn, "pnl, equity, n_long, n_short and summary are all NULL");
        if (annualization <= 0)
            return refuse(fn, "annualization = " + std::to_string(annualization) + " is not positive");
        int64_t lanes = 0;
        int32_t lo = 0, hi = 0;
        for (int32_t w = 0; w < world; ++w) {
            const bt_pf_summary& s = summaries[w];
            if (s.n_lanes < 0 || s.first_bar < 0 || s.n_bars < 0 || (int64_t)s.first_bar + s.n_bars > T)
                return refuse(fn, "part " + std::to_string(w) + " covers bars [" + std::to_string(s.first_bar) + ", " +
                                      std::to_string((int64_t)s.first_bar + s.n_bars) + ") of T = " + std::to_string(T) +
                                      " with " + std::to_string(s.n_lanes) + " entries");
            if (s.n_lanes == 0) continue;
            lo = lanes ? std::min(lo, s.first_bar) : s.first_bar;
            hi = lanes ? std::max(hi, s.first_bar + s.n_bars) : s.first_bar + s.n_bars;
            lanes += s.n_lanes;
        }
        if (lanes > BT_PORTFOLIO_MAX)
            return refuse(fn, "the parts hold " + std::to_string(lanes) + " entries, above " + std::to_string(BT_PORTFOLIO_MAX));
        std::vector<int64_t> p((size_t)T, 0);
        std::vector<int32_t> nl((size_t)T, 0), ns((size_t)T, 0);
        for (int32_t w = 0; w < world; ++w)
            for (int32_t t = 0; t < T; ++t) {
                const size_t at = (size_t)w * (size_t)T + (size_t)t;
                p[t] += pnl[at];
                nl[t] += n_long[at];
                ns[t] += n_short[at];
            }
        bt::portfolio_finish_host(T, (int32_t)lanes, lo, hi, p.data(), nl.data(), ns.data(),
                                  std::sqrt((double)annualization), out_equity, summary);
        give(T, p, nl, ns, out_pnl, out_long, out_short);
        return 0;
    } catch (const std::exception& x) {
        return refuse(fn, std::string("exception: ") + x.what());
    }
}

}  // extern "C"
