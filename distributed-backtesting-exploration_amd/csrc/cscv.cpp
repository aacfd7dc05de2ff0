// cscv.cpp — the probability of backtest overfitting on the host (docs/cscv_spec.md): the argument
// rules of bt_cscv / bt_cscv_of and bt_cscv_host, the scalar restatement of what k_cscv.hip
// computes from fold records. Written from the spec with the compiler's __int128: every
// combination is found by counting the bits of every K-bit word, and both halves are summed fold by
// fold (the kernel takes masks from the planner's table and the second half as total minus first),
// so that the two check each other. Plain C++: no HIP call, builds with any host compiler.
#include "cscv.h"

#include <cmath>
#include <cstring>
#include <exception>
#include <vector>

#include "walkfwd.h"

namespace bt {

std::string cscv_refusal(int64_t K, const int32_t* bounds, bool want_groups, bool want_hist, bool want_picks, int64_t G) {
    if (K < 2 || K > BT_CSCV_MAX_FOLDS)
        return "K = " + std::to_string(K) + " outside [2, " + std::to_string(BT_CSCV_MAX_FOLDS) + "]";
    if (K % 2) return "K = " + std::to_string(K) + " is odd";
    if (bounds) {   // the walk-forward rule of the bounds, with outputs that rule accepts
        const std::string why = walkfwd_refusal(K, bounds, 1, false, true, false, 0, 1);
        if (!why.empty()) return why;
    }
    if (!want_groups && !want_hist && !want_picks) return "groups, hist and picks are all NULL";
    const int64_t C = cscv_combos((int32_t)K);
    if (want_picks && G * C > kCscvPicksMax)
        return "G*C = " + std::to_string(G) + "*" + std::to_string(C) + " exceeds 2^22 pick records";
    return "";
}

std::string cscv_folds_refusal(int64_t G, int64_t P, int32_t K, const bt_fold* folds) {
    if (P < 1) return "P = " + std::to_string(P) + " is below 1";
    if (G < 0) return "G = " + std::to_string(G) + " is negative";
    if (G > 0 && !folds) return "folds are required";
    const i128 lim = (i128)1 << kCscvSumBits;
    for (int64_t g = 0; g < G; ++g) {
        const bt_fold* grp = folds + (size_t)g * (size_t)P * (size_t)K;
        const std::string at0 = " (group " + std::to_string(g) + ", lane ";
        int64_t n = 0;
        for (int32_t k = 0; k < K; ++k) {
            const bt_fold& f = grp[k];
            const std::string at = at0 + "0, fold " + std::to_string(k) + ")";
            if (f.first_bar < 0) return "first_bar = " + std::to_string(f.first_bar) + " is negative" + at;
            if (f.n_bars < 0) return "n_bars = " + std::to_string(f.n_bars) + " is negative" + at;
            n += fold_ret_bars(f);
        }
        if (n >= INT32_MAX)
            return std::to_string(n) + " return bars in group " + std::to_string(g) + " exceed 2^31 - 2";
        for (int64_t p = 0; p < P; ++p)
            for (int32_t k = 0; k < K; ++k) {
                const bt_fold& f = grp[(size_t)p * (size_t)K + (size_t)k];
                const std::string at = at0 + std::to_string(p) + ", fold " + std::to_string(k) + ")";
                if (f.first_bar != grp[k].first_bar || f.n_bars != grp[k].n_bars)
                    return "first_bar, n_bars = " + std::to_string(f.first_bar) + ", " + std::to_string(f.n_bars) +
                           " differ from lane 0's " + std::to_string(grp[k].first_bar) + ", " +
                           std::to_string(grp[k].n_bars) + at;
                const i128 s1 = wide_join(f.s1_lo, f.s1_hi), s2 = wide_join(f.s2_lo, f.s2_hi);
                if (s2 < 0 || s2 >= lim) return std::string("s2 outside [0, 2^120)") + at;
                if (s1 >= lim || s1 <= -lim) return std::string("|s1| is 2^120 or more") + at;
            }
    }
    return "";
}

}  // namespace bt

namespace {

using bt::fold_ret_bars;
using bt::host_sharpe;
using bt::host_sharpe_key;
using bt::i128;
using bt::refuse;
using bt::wide_join;

// One group's results from its fold records grp[p * K + k]; hist (2P - 1 counters, zeroed by the
// caller) and picks (C records) may be NULL.
void group_cscv(const bt_fold* grp, int32_t P, int32_t K, double sqrt_ann, bt_cscv_group& out, uint32_t* hist,
                bt_cscv_pick* picks) {
    std::vector<uint64_t> kin((size_t)P), kout((size_t)P);
    std::vector<double> sin((size_t)P), sout((size_t)P);
    std::vector<char> neg((size_t)P);
    int64_t c = 0;
    for (uint32_t m = 0; m < (1u << K); ++m) {        // increasing numeric order
        if (__builtin_popcount(m) != K / 2) continue;
        bt_cscv_pick pk{-1, 0, 0.0, 0.0};
        int64_t n_is = 0, n_oos = 0;
        for (int32_t k = 0; k < K; ++k) ((m >> k) & 1 ? n_is : n_oos) += fold_ret_bars(grp[k]);
        if (n_is == 0 || n_oos == 0) {
            ++out.n_dead;
        } else {
            for (int32_t p = 0; p < P; ++p) {
                i128 a1 = 0, a2 = 0, b1 = 0, b2 = 0;
                for (int32_t k = 0; k < K; ++k) {
                    const bt_fold& f = grp[(size_t)p * (size_t)K + (size_t)k];
                    if ((m >> k) & 1) {
                        a1 += wide_join(f.s1_lo, f.s1_hi);
                        a2 += wide_join(f.s2_lo, f.s2_hi);
                    } else {
                        b1 += wide_join(f.s1_lo, f.s1_hi);
                        b2 += wide_join(f.s2_lo, f.s2_hi);
                    }
                }
                sin[p] = host_sharpe(a1, a2, n_is, sqrt_ann);
                sout[p] = host_sharpe(b1, b2, n_oos, sqrt_ann);
                kin[p] = host_sharpe_key(sin[p]);
                kout[p] = host_sharpe_key(sout[p]);
                neg[p] = b1 < 0;
            }
            int32_t best = 0;
            for (int32_t p = 1; p < P; ++p)
                if (kin[p] > kin[best]) best = p;     // ties stay with the lower p
            int32_t below = 0, equal = 0, tied = 0;
            for (int32_t q = 0; q < P; ++q) {
                below += kout[q] < kout[best];
                equal += q != best && kout[q] == kout[best];
                tied += q != best && kin[q] == kin[best];
            }
            pk = bt_cscv_pick{best, 2 * below + equal, sin[best], sout[best]};
            ++out.n_live;
            out.n_overfit += pk.r2 <= P - 1;
            out.n_loss += neg[best] != 0;
            out.n_tied += tied > 0;
            if (hist) ++hist[pk.r2];
        }
        if (picks) picks[c] = pk;
        ++c;
    }
}

}  // namespace

extern "C" {

int32_t bt_cscv_host(int32_t G, int32_t P, int32_t K, const bt_fold* folds, const int32_t* sym_ids,
                     int64_t annualization, bt_cscv_group* groups, uint32_t* hist, bt_cscv_pick* picks) {
    const char* fn = "bt_cscv_host";
    try {
        std::string why = bt::cscv_refusal(K, nullptr, groups != nullptr, hist != nullptr, picks != nullptr,
                                           G > 0 ? G : 0);
        if (why.empty()) why = bt::cscv_folds_refusal(G, P, K, folds);
        if (!why.empty()) return refuse(fn, why);
        if (annualization <= 0)
            return refuse(fn, "annualization = " + std::to_string(annualization) + " is not positive");
        const double sqrt_ann = std::sqrt((double)annualization);
        const size_t C = (size_t)bt::cscv_combos(K), H = 2 * (size_t)P - 1;
        if (hist) memset(hist, 0, (size_t)G * H * sizeof(uint32_t));
        for (int32_t g = 0; g < G; ++g) {
            bt_cscv_group grp;
            memset(&grp, 0, sizeof grp);
            grp.sym = sym_ids ? sym_ids[g] : g;
            grp.n_lanes = P;
            group_cscv(folds + (size_t)g * (size_t)P * (size_t)K, P, K, sqrt_ann, grp, hist ? hist + (size_t)g * H : nullptr,
                       picks ? picks + (size_t)g * C : nullptr);
            if (groups) groups[g] = grp;
        }
        return 0;
    } catch (const std::exception& x) {
        return refuse(fn, std::string("exception: ") + x.what());
    }
}

}  // extern "C"
