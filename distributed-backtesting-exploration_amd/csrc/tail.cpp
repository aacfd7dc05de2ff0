// tail.cpp — the tail-risk figures on the host (docs/tail_spec.md): the argument rules of bt_tail
// and bt_tail_of, and bt_tail_host, the scalar restatement from replayed curves. Written from the
// spec, bar by bar with the compiler's __int128 and a sort of a copy of the row; it shares no code
// with k_tail.hip but the split of an int128 into its words (host_common.h), so that the two check
// each other. Plain C++: no HIP call, builds with any host compiler.
#include "tail.h"

#include <algorithm>
#include <cstring>
#include <exception>
#include <vector>

namespace bt {

std::string tail_levels_refusal(int64_t Q, const int32_t* alpha_ppm) {
    if (Q < 1 || Q > BT_TAIL_LEVELS_MAX)
        return "Q = " + std::to_string(Q) + " outside [1, " + std::to_string(BT_TAIL_LEVELS_MAX) + "]";
    if (!alpha_ppm) return "alpha_ppm is NULL";
    for (int64_t j = 0; j < Q; ++j)
        if (alpha_ppm[j] < 1 || alpha_ppm[j] > BT_TAIL_PPM_MAX)
            return "level " + std::to_string(j) + ": alpha_ppm = " + std::to_string(alpha_ppm[j]) + " outside [1, " +
                   std::to_string(BT_TAIL_PPM_MAX) + "]";
    return "";
}

namespace {

std::string mode_window_refusal(int64_t from_bar, int64_t to_bar, int64_t mode) {
    if (mode != BT_TAIL_ALL && mode != BT_TAIL_HELD)
        return "mode = " + std::to_string(mode) + " is neither BT_TAIL_ALL (0) nor BT_TAIL_HELD (1)";
    if (from_bar < 0 || to_bar < 0 || ((from_bar != 0 || to_bar != 0) && to_bar <= from_bar))
        return "window [" + std::to_string(from_bar) + ", " + std::to_string(to_bar) +
               ") is empty or negative (0, 0 is the whole row)";
    return "";
}

}  // namespace

std::string tail_refusal(bool have_dataset, int64_t n, bool have_lanes, int64_t from_bar, int64_t to_bar, int64_t mode,
                         int64_t Q, const int32_t* alpha_ppm, bool have_recs, bool have_q, int64_t max_bars) {
    if (!have_dataset) return "no dataset loaded";
    if (have_lanes) {
        if (n < 1 || n > BT_TAIL_MAX)
            return "n = " + std::to_string(n) + " outside [1, " + std::to_string(BT_TAIL_MAX) + "]";
    } else if (n != 0) {
        return "n = " + std::to_string(n) + " with lanes == NULL (all-lanes mode takes n = 0)";
    }
    std::string why = tail_levels_refusal(Q, alpha_ppm);
    if (why.empty()) why = mode_window_refusal(from_bar, to_bar, mode);
    if (!why.empty()) return why;
    if (!have_recs && !have_q) return "recs_out and q_out are both NULL";
    if (max_bars > BT_TAIL_BARS_MAX)
        return "T = " + std::to_string(max_bars) + " bars of the longest row exceed " + std::to_string(BT_TAIL_BARS_MAX);
    return "";
}

std::string tail_of_refusal(int64_t n, int64_t T, bool have_d, int64_t Q, const int32_t* alpha_ppm, bool have_recs,
                            bool have_q) {
    if (n < 1 || n > BT_TAIL_MAX) return "n = " + std::to_string(n) + " outside [1, " + std::to_string(BT_TAIL_MAX) + "]";
    if (T < 1 || T > BT_TAIL_BARS_MAX)
        return "T = " + std::to_string(T) + " outside [1, " + std::to_string(BT_TAIL_BARS_MAX) + "]";
    if (!have_d) return "d is NULL";
    const std::string why = tail_levels_refusal(Q, alpha_ppm);
    if (!why.empty()) return why;
    if (!have_recs && !have_q) return "recs_out and q_out are both NULL";
    return "";
}

int32_t tail_longest(int32_t from_bar, int32_t to_bar, int32_t longest) {
    const int64_t to = from_bar == 0 && to_bar == 0 ? (int64_t)longest : std::min<int64_t>(to_bar, longest);
    return (int32_t)std::max<int64_t>(to - from_bar, 0);
}

std::string tail_row_refusal(int64_t longest_n, size_t row_bytes, size_t lds_row_bytes) {
    return "a row of " + std::to_string(longest_n) + " counted bars (" + std::to_string(row_bytes) +
           " bytes) does not fit the " + std::to_string(lds_row_bytes) + " bytes of LDS a workgroup keeps for it";
}

std::string tail_budget_refusal(bool all_lanes, size_t need_bytes, size_t budget) {
    return std::string("the staging of one ") + (all_lanes ? "dataset row" : "lane") + " (" + std::to_string(need_bytes) +
           " bytes) exceeds the budget of " +
           std::to_string(budget) + " bytes";
}

}  // namespace bt

extern "C" {

int32_t bt_tail_host(int32_t n, const int64_t* equity, const int8_t* pos, const int32_t* n_bars, int64_t stride,
                     int32_t from_bar, int32_t to_bar, int32_t mode, int32_t Q, const int32_t* alpha_ppm,
                     bt_tail_rec* recs_out, bt_tail_q* q_out) {
    using bt::i128;
    using bt::refuse;
    typedef unsigned __int128 u128;
    const char* fn = "bt_tail_host";
    try {
        if (n < 0) return refuse(fn, "n = " + std::to_string(n) + " is negative");
        std::string why = bt::tail_levels_refusal(Q, alpha_ppm);
        if (why.empty()) why = bt::mode_window_refusal(from_bar, to_bar, mode);
        if (!why.empty()) return refuse(fn, why);
        if (!recs_out && !q_out) return refuse(fn, "recs_out and q_out are both NULL");
        int32_t b_max = 0;
        why = bt::curves_refusal(n, equity && n_bars, "equity and n_bars", n_bars, stride, "lane", b_max);
        if (!why.empty()) return refuse(fn, why);
        if (mode == BT_TAIL_HELD && n > 0 && !pos) return refuse(fn, "pos is required with mode BT_TAIL_HELD");
        if (b_max > BT_TAIL_BARS_MAX)
            return refuse(fn, "T = " + std::to_string(b_max) + " bars of the longest row exceed " +
                                  std::to_string(BT_TAIL_BARS_MAX));
        const bool whole = from_bar == 0 && to_bar == 0;
        std::vector<int64_t> row;
        for (int32_t i = 0; i < n; ++i) {
            const int64_t* E = equity + (size_t)i * (size_t)stride;
            const int8_t* ps = pos ? pos + (size_t)i * (size_t)stride : nullptr;
            const int32_t end = whole ? n_bars[i] : std::min(to_bar, n_bars[i]);
            bt_tail_rec r;
            memset(&r, 0, sizeof r);
            r.min_bar = r.max_bar = -1;
            i128 s2 = 0, s2n = 0, s3 = 0;
            u128 s4 = 0;
            uint64_t s4_top = 0;
            row.clear();
            for (int32_t t = from_bar; t < end; ++t) {
                r.n_window += 1;
                if (mode == BT_TAIL_HELD && !(t >= 1 && ps[t - 1] != 0)) continue;
                const int64_t d = E[t] - (t > 0 ? E[t - 1] : 0);
                if (d <= -(1LL << 31) || d >= (1LL << 31))
                    return refuse(fn, "increment " + std::to_string(d) + " at bar " + std::to_string(t) + " of lane " +
                                          std::to_string(i) + " outside the domain |d| < 2^31");
                row.push_back(d);
                if (r.n == 0 || d < r.min_d) r.min_d = d, r.min_bar = t;
                if (r.n == 0 || d > r.max_d) r.max_d = d, r.max_bar = t;
                r.n += 1;
                r.n_pos += d > 0, r.n_neg += d < 0;
                r.s1 += d;
                const i128 dd = (i128)d * d;
                s2 += dd;
                s3 += dd * d;
                const u128 d4 = (u128)dd * (u128)dd, before = s4;
                s4 += d4;
                if (s4 < before) ++s4_top;
                if (d < 0) r.s1_neg += d, s2n += dd;
            }
            r.s2 = bt::wide_rec(s2), r.s2_neg = bt::wide_rec(s2n), r.s3 = bt::wide_rec(s3);
            r.s4[0] = (uint64_t)s4, r.s4[1] = (uint64_t)(s4 >> 64), r.s4[2] = s4_top;
            if (recs_out) recs_out[i] = r;
            if (!q_out) continue;
            std::sort(row.begin(), row.end());
            for (int32_t j = 0; j < Q; ++j) {
                bt_tail_q q;
                memset(&q, 0, sizeof q);
                if (r.n > 0) {
                    const int64_t k = ((int64_t)r.n * alpha_ppm[j] + 999999) / 1000000;
                    q.k = (int32_t)k;
                    q.var = row[(size_t)k - 1];
                    for (int64_t u = 0; u < k; ++u) q.es_sum += row[(size_t)u];
                    q.n_lt = (int32_t)(std::lower_bound(row.begin(), row.end(), q.var) - row.begin());
                }
                q_out[(size_t)i * (size_t)Q + (size_t)j] = q;
            }
        }
        return 0;
    } catch (const std::exception& x) {
        return refuse(fn, std::string("exception: ") + x.what());
    }
}

}  // extern "C"
