// ddboot.cpp — the drawdown bootstrap on the host (docs/drawdown_spec.md): the argument rules of
// bt_drawdown_boot / bt_drawdown_boot_of and bt_drawdown_boot_host, the scalar restatement from
// replayed equity curves. It adds the drawn bars one by one, bar after bar with the index wrapped
// at T, and keeps the running sum, its peak and the largest distance below it: no prefix row, no
// block summary and no composition, so that it shares nothing with k_ddboot.hip and the two check
// each other. The quantiles come from a sort. Plain C++: no HIP call, builds with any host compiler.
#include "ddboot.h"

#include <algorithm>
#include <exception>
#include <vector>

namespace bt {

std::string dd_levels_refusal(int64_t Q, const int32_t* alpha_ppm, int64_t R, const int64_t* limits) {
    if (Q < 0 || Q > BT_DD_LEVELS_MAX)
        return "Q = " + std::to_string(Q) + " outside [0, " + std::to_string(BT_DD_LEVELS_MAX) + "]";
    if (R < 0 || R > BT_DD_LIMITS_MAX)
        return "R = " + std::to_string(R) + " outside [0, " + std::to_string(BT_DD_LIMITS_MAX) + "]";
    if (Q > 0 && !alpha_ppm) return "alpha_ppm is NULL";
    for (int64_t j = 0; j < Q; ++j)
        if (alpha_ppm[j] < 1 || alpha_ppm[j] > kDdPpmMax)
            return "level " + std::to_string(j) + ": alpha_ppm = " + std::to_string(alpha_ppm[j]) + " outside [1, " +
                   std::to_string(kDdPpmMax) + "]";
    if (R > 0 && !limits) return "limits is NULL";
    for (int64_t r = 0; r < R; ++r)
        if (limits[r] < 0) return "limit " + std::to_string(r) + ": " + std::to_string(limits[r]) + " is negative";
    return "";
}

std::string dd_refusal(const DdCall& c) {
    if (!c.have_engine) return "null engine";
    if (!c.staged && !c.have_dataset) return "no dataset loaded";
    const bool list = c.staged || c.have_lanes;
    if (list) {
        if (c.n < 1 || c.n > BT_BOOT_MAX)
            return "n = " + std::to_string(c.n) + " outside [1, " + std::to_string(BT_BOOT_MAX) + "]";
        if (c.staged && !c.have_lanes) return "d is required";
    } else if (c.n != 0) {
        return "n = " + std::to_string(c.n) + " with lanes == NULL (all-lanes mode takes n = 0)";
    }
    if (c.from_bar < 0) return "from_bar = " + std::to_string(c.from_bar) + " is negative";
    if (c.B < 1 || c.B > BT_BOOT_MAX_RESAMPLES)
        return "B = " + std::to_string(c.B) + " outside [1, " + std::to_string(BT_BOOT_MAX_RESAMPLES) + "]";
    if (c.L < 1 || c.L > kBootMaxT) return "L = " + std::to_string(c.L) + " outside [1, " + std::to_string(kBootMaxT) + "]";
    const std::string why = dd_levels_refusal(c.Q, c.alpha_ppm, c.R, c.limits);
    if (!why.empty()) return why;
    if (!c.have_rec && !(c.have_q && c.Q > 0) && !(c.have_reach && c.R > 0) && !c.have_raw)
        return "lanes_out, q_out, reach_out and raw_out are all NULL";
    if (!list && c.have_raw) return "raw_out given in all-lanes mode: it must be NULL";
    return "";
}

std::string dd_budget_refusal(size_t need_bytes, size_t budget) {
    if (need_bytes <= budget) return "";
    return "the call needs " + std::to_string(need_bytes) + " bytes of device staging, above the budget of " +
           std::to_string(budget) + " bytes";
}

std::string dd_row_refusal(int64_t T, size_t row_bytes, size_t limit_bytes) {
    if (row_bytes <= limit_bytes) return "";
    return "the prefix row and block tables of T = " + std::to_string(T) + " bars (" + std::to_string(row_bytes) +
           " bytes) do not fit the LDS row limit of " + std::to_string(limit_bytes) + " bytes (bt_set_ddboot_row mode 1)";
}

}  // namespace bt

using bt::i128;
using bt::refuse;
using bt::wide_rec;

extern "C" {

int32_t bt_drawdown_boot_host(int32_t n, const int64_t* equity, const int32_t* n_bars, int64_t stride, int32_t from_bar,
                              int32_t to_bar, int32_t B, int32_t L, uint64_t seed, int32_t Q, const int32_t* alpha_ppm,
                              int32_t R, const int64_t* limits, bt_dd_lane* lanes_out, int64_t* q_out,
                              int64_t* reach_out, int64_t* raw_out) {
    const char* fn = "bt_drawdown_boot_host";
    try {
        const bt::DdCall call{true,  true, false, true, n, from_bar, B, L, Q, alpha_ppm, R, limits, lanes_out != nullptr,
                              q_out != nullptr, reach_out != nullptr, raw_out != nullptr};
        std::string why = bt::dd_refusal(call);
        if (!why.empty()) return refuse(fn, why);
        int32_t b_max = 0, T = 0;
        why = bt::curves_refusal(n, equity && n_bars, "equity and n_bars", n_bars, stride, "lane", b_max);
        if (why.empty()) why = bt::boot_window(from_bar, to_bar, b_max, T);
        if (!why.empty()) return refuse(fn, why);
        std::vector<int64_t> S((size_t)n, 0);
        const std::vector<int64_t> d = bt::curve_increments(n, equity, n_bars, stride, from_bar, T, S.data());
        for (size_t k = 0; k < d.size(); ++k)
            if (d[k] <= -(1LL << 31) || d[k] >= (1LL << 31))
                return refuse(fn, "increment " + std::to_string(d[k]) + " at bar " + std::to_string(from_bar + (int64_t)(k % (size_t)T)) +
                                      " of lane " + std::to_string(k / (size_t)T) + " outside the domain |d| < 2^31");
        const int32_t Lp = std::min(L, T), K = (T + Lp - 1) / Lp;
        // the drawn bars of one resample, in drawing order: drawn again for every lane, so that the call
        // holds T bars and B values whatever n and B are
        std::vector<int32_t> bars((size_t)T);
        auto draw_bars = [&](int32_t b) {
            size_t m = 0;
            for (int32_t j = 0; j < K; ++j) {
                int32_t at = (int32_t)(bt::boot_draw(seed, (uint64_t)b, (uint64_t)j) % (uint64_t)T);
                const int32_t len = j < K - 1 ? Lp : T - (K - 1) * Lp;
                for (int32_t u = 0; u < len; ++u) {
                    bars[m++] = at;
                    at = at + 1 == T ? 0 : at + 1;
                }
            }
        };
        std::vector<int64_t> star((size_t)B);
        for (int32_t i = 0; i < n; ++i) {
            const int64_t* row = d.data() + (size_t)i * (size_t)T;
            int64_t x = 0, peak = 0, mdd = 0;
            for (int32_t u = 0; u < T; ++u) {
                x += row[u];
                peak = std::max(peak, x);
                mdd = std::max(mdd, peak - x);
            }
            bt_dd_lane rec{};
            rec.sum = S[(size_t)i], rec.mdd = mdd;
            i128 m1 = 0, m2 = 0;
            for (int32_t b = 0; b < B; ++b) {
                draw_bars(b);
                const int32_t* at = bars.data();
                int64_t xs = 0, pk = 0, md = 0;
                for (int32_t u = 0; u < T; ++u) {
                    xs += row[at[u]];
                    pk = std::max(pk, xs);
                    md = std::max(md, pk - xs);
                }
                star[(size_t)b] = md;
                m1 += (i128)md;
                m2 += (i128)md * (i128)md;
                rec.n_ge += md >= mdd ? 1 : 0;
                rec.min_star = b == 0 ? md : std::min(rec.min_star, md);
                rec.max_star = b == 0 ? md : std::max(rec.max_star, md);
            }
            rec.m1 = wide_rec(m1), rec.m2 = wide_rec(m2);
            if (lanes_out) lanes_out[i] = rec;
            if (raw_out) std::copy(star.begin(), star.end(), raw_out + (size_t)i * (size_t)B);
            if (reach_out)
                for (int32_t r = 0; r < R; ++r) {
                    int64_t c = 0;
                    for (int32_t b = 0; b < B; ++b) c += star[(size_t)b] >= limits[r] ? 1 : 0;
                    reach_out[(size_t)i * (size_t)R + (size_t)r] = c;
                }
            if (q_out && Q > 0) {
                std::sort(star.begin(), star.end());
                for (int32_t j = 0; j < Q; ++j)
                    q_out[(size_t)i * (size_t)Q + (size_t)j] = star[(size_t)bt::dd_rank(B, alpha_ppm[j]) - 1];
            }
        }
        return 0;
    } catch (const std::exception& x) {
        return refuse(fn, std::string("exception: ") + x.what());
    }
}

}  // extern "C"
