// bootstrap.cpp — the bootstrap reality check on the host (docs/bootstrap_spec.md): the argument
// rules of bt_bootstrap / bt_bootstrap_of and bt_bootstrap_host, the scalar restatement from
// replayed equity curves. It adds the drawn bars themselves, T additions per lane and resample in
// __int128, bar after bar with the index wrapped at T: no prefix row and no difference of two
// prefix values, so that it shares nothing with k_boot.hip and the two check each other. Plain
// C++: no HIP call, builds with any host compiler.
#include "bootstrap.h"

#include <algorithm>
#include <exception>
#include <vector>

namespace bt {

std::string boot_refusal(const BootCall& c) {
    if (!c.have_engine) return "null engine";
    if (!c.staged && !c.have_dataset) return "no dataset loaded";
    const bool list = c.staged || c.have_lanes;
    if (list) {
        if (c.n < 1 || c.n > BT_BOOT_MAX)
            return "n = " + std::to_string(c.n) + " outside [1, " + std::to_string(BT_BOOT_MAX) + "]";
        if (c.staged && !c.have_lanes) return "d is required";
        if (!c.goff) {
            if (c.G != 0 && c.G != 1)
                return "G = " + std::to_string(c.G) + " with goff == NULL (one group: G is 0 or 1)";
        } else {
            const std::string why = boot_groups_refusal(c.n, c.G, c.goff);
            if (!why.empty()) return why;
        }
    } else {
        if (c.n != 0) return "n = " + std::to_string(c.n) + " with lanes == NULL (all-lanes mode takes n = 0)";
        if (c.goff || c.G != 0)
            return "G = " + std::to_string(c.G) + (c.goff ? " and goff" : "") +
                   " given in all-lanes mode (one group per dataset row: G = 0, goff == NULL)";
    }
    if (c.from_bar < 0) return "from_bar = " + std::to_string(c.from_bar) + " is negative";
    if (c.B < 1 || c.B > BT_BOOT_MAX_RESAMPLES)
        return "B = " + std::to_string(c.B) + " outside [1, " + std::to_string(BT_BOOT_MAX_RESAMPLES) + "]";
    if (c.L < 1 || c.L > kBootMaxT) return "L = " + std::to_string(c.L) + " outside [1, " + std::to_string(kBootMaxT) + "]";
    if (!c.any_output) return "groups, lanes, vmax and boot are all NULL";
    if (!list && c.want_boot) return "boot given in all-lanes mode: it must be NULL";
    return "";
}

std::string boot_groups_refusal(int64_t n, int64_t G, const int32_t* goff) {
    if (G < 1 || G > n) return "G = " + std::to_string(G) + " outside [1, n = " + std::to_string(n) + "]";
    if (goff[0] != 0) return "goff[0] = " + std::to_string(goff[0]) + " is not 0";
    for (int64_t g = 0; g < G; ++g)
        if (goff[g + 1] <= goff[g])
            return "goff[" + std::to_string(g + 1) + "] = " + std::to_string(goff[g + 1]) + " is not above goff[" +
                   std::to_string(g) + "] = " + std::to_string(goff[g]) + " (group " + std::to_string(g) + " is empty)";
    if (goff[G] != n) return "goff[" + std::to_string(G) + "] = " + std::to_string(goff[G]) + " is not n = " + std::to_string(n);
    return "";
}

std::string boot_window(int64_t from_bar, int64_t to_bar, int64_t b_max, int32_t& T) {
    const int64_t t = (from_bar == 0 && to_bar == 0) ? b_max : to_bar - from_bar;
    T = (int32_t)std::max<int64_t>(0, std::min<int64_t>(t, INT32_MAX));
    if (t < 1 || t > kBootMaxT)
        return "T = " + std::to_string(t) + " bars of the window [" + std::to_string(from_bar) + ", " +
               std::to_string(from_bar + t) + ") outside [1, " + std::to_string(kBootMaxT) + "]";
    return "";
}

std::string boot_budget_refusal(size_t need_bytes, size_t budget) {
    if (need_bytes <= budget) return "";
    return "the call needs " + std::to_string(need_bytes) + " bytes of device staging, above the budget of " +
           std::to_string(budget) + " bytes";
}

std::string boot_row_refusal(int64_t T, size_t row_bytes, size_t limit_bytes) {
    if (row_bytes <= limit_bytes) return "";
    return "a prefix row of T + 1 = " + std::to_string(T + 1) + " words (" + std::to_string(row_bytes) +
           " bytes) does not fit the LDS row limit of " + std::to_string(limit_bytes) + " bytes (bt_set_boot_row mode 1)";
}

}  // namespace bt

using bt::i128;
using bt::refuse;
using bt::wide_rec;

extern "C" {

int32_t bt_bootstrap_host(int32_t n, const int64_t* equity, const int32_t* n_bars, int64_t stride, int32_t G,
                          const int32_t* goff, int32_t from_bar, int32_t to_bar, int32_t B, int32_t L,
                          uint64_t seed, bt_boot_group* groups_out, bt_boot_lane* lanes_out, int64_t* vmax_out,
                          int64_t* boot_out) {
    const char* fn = "bt_bootstrap_host";
    try {
        const bt::BootCall call{true, true, false, true, n, G, goff, from_bar, to_bar, B, L,
                                groups_out || lanes_out || vmax_out || boot_out, boot_out != nullptr};
        std::string why = bt::boot_refusal(call);
        if (!why.empty()) return refuse(fn, why);
        int32_t b_max = 0, T = 0;
        why = bt::curves_refusal(n, equity && n_bars, "equity and n_bars", n_bars, stride, "lane", b_max);
        if (why.empty()) why = bt::boot_window(from_bar, to_bar, b_max, T);
        if (!why.empty()) return refuse(fn, why);
        const int32_t one[2] = {0, n};
        if (!goff) goff = one, G = 1;

        std::vector<int64_t> S((size_t)n, 0);
        const std::vector<int64_t> d = bt::curve_increments(n, equity, n_bars, stride, from_bar, T, S.data());
        const int32_t Lp = std::min(L, T), K = (T + Lp - 1) / Lp;
        std::vector<i128> m1((size_t)n, 0), m2((size_t)n, 0), star((size_t)n);
        std::vector<int64_t> nonpos((size_t)n, 0), nge((size_t)G, 0), best((size_t)G);
        std::vector<int32_t> best_lane((size_t)G);
        for (int32_t g = 0; g < G; ++g) {
            best[(size_t)g] = S[(size_t)goff[g]], best_lane[(size_t)g] = 0;
            for (int32_t i = goff[g] + 1; i < goff[g + 1]; ++i)
                if (S[(size_t)i] > best[(size_t)g]) best[(size_t)g] = S[(size_t)i], best_lane[(size_t)g] = i - goff[g];
        }
        std::vector<int32_t> bars((size_t)T);   // the drawn bars of one resample, in drawing order
        for (int32_t b = 0; b < B; ++b) {
            int32_t m = 0;
            for (int32_t j = 0; j < K; ++j) {
                int32_t at = (int32_t)(bt::boot_draw(seed, (uint64_t)b, (uint64_t)j) % (uint64_t)T);
                const int32_t len = j < K - 1 ? Lp : T - (K - 1) * Lp;
                for (int32_t u = 0; u < len; ++u) {
                    bars[(size_t)m++] = at;
                    at = at + 1 == T ? 0 : at + 1;
                }
            }
            for (int32_t i = 0; i < n; ++i) {
                const int64_t* row = d.data() + (size_t)i * (size_t)T;
                i128 s = 0;
                for (int32_t u = 0; u < T; ++u) s += (i128)row[bars[(size_t)u]];
                star[(size_t)i] = s;
                m1[(size_t)i] += s;
                m2[(size_t)i] += s * s;
                nonpos[(size_t)i] += s <= 0 ? 1 : 0;
                if (boot_out) boot_out[(size_t)i * (size_t)B + (size_t)b] = (int64_t)s;
            }
            for (int32_t g = 0; g < G; ++g) {
                i128 v = star[(size_t)goff[g]] - (i128)S[(size_t)goff[g]];
                for (int32_t i = goff[g] + 1; i < goff[g + 1]; ++i)
                    v = std::max(v, star[(size_t)i] - (i128)S[(size_t)i]);
                if (vmax_out) vmax_out[(size_t)g * (size_t)B + (size_t)b] = (int64_t)v;
                nge[(size_t)g] += v >= (i128)best[(size_t)g] ? 1 : 0;
            }
        }
        if (lanes_out)
            for (int32_t i = 0; i < n; ++i)
                lanes_out[i] = bt_boot_lane{S[(size_t)i], nonpos[(size_t)i], wide_rec(m1[(size_t)i]), wide_rec(m2[(size_t)i])};
        if (groups_out)
            for (int32_t g = 0; g < G; ++g)
                groups_out[g] = bt_boot_group{best[(size_t)g], best_lane[(size_t)g], goff[g + 1] - goff[g], nge[(size_t)g]};
        return 0;
    } catch (const std::exception& x) {
        return refuse(fn, std::string("exception: ") + x.what());
    }
}

}  // extern "C"
