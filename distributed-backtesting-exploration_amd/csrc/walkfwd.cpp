// walkfwd.cpp — the walk-forward selection on the host (docs/walkforward_spec.md):
// bt_walk_forward_host, the scalar restatement of what k_walkfwd.hip's selection computes on the
// device from the fold records, and the per-row totals, which the device path uses too. Written
// from the spec with the compiler's __int128 and shares no code with the kernels but the split of
// an int128 into its words (host_common.h), so that the two check each other. Plain C++: no HIP
// call, builds with any host compiler.
#include "walkfwd.h"

#include <cmath>
#include <cstring>
#include <exception>
#include <vector>

namespace bt {

std::string walkfwd_refusal(int64_t K, const int32_t* bounds, int64_t train, bool want_folds,
                            bool want_steps, bool want_total, int64_t S, int64_t P) {
    if (K < 1) return "K = " + std::to_string(K) + " is below 1";
    if (bounds) {
        if (bounds[0] < 0) return "bounds[0] = " + std::to_string(bounds[0]) + " is negative";
        for (int64_t k = 0; k < K; ++k)
            if (bounds[k + 1] <= bounds[k])
                return "bounds[" + std::to_string(k + 1) + "] = " + std::to_string(bounds[k + 1]) +
                       " does not exceed bounds[" + std::to_string(k) + "] = " + std::to_string(bounds[k]);
    }
    if (train < 0 || train > K - 1)
        return "train = " + std::to_string(train) + " outside [0, " + std::to_string(K - 1) + "]";
    if (!want_folds && !want_steps && !want_total) return "folds, steps and total are all NULL";
    if ((want_steps || want_total) && K < 2)
        return "K = " + std::to_string(K) + ": steps and total need at least 2 folds";
    if (want_folds && (S > kWalkfwdFoldsMax || P > kWalkfwdFoldsMax || S * P > kWalkfwdFoldsMax ||
                       S * P * K > kWalkfwdFoldsMax))
        return "S*P*K = " + std::to_string(S) + "*" + std::to_string(P) + "*" + std::to_string(K) +
               " exceeds 2^22 fold records";
    return "";
}

}  // namespace bt

namespace {

using bt::i128;
using bt::refuse;
using bt::wide_join;
using bt::wide_split;

// The shared host Sharpe, its key and a record's return bars (host_common.h).
uint64_t sharpe_key(double x) { return bt::host_sharpe_key(x); }
double sharpe_of(i128 s1, i128 s2, int64_t n, double sqrt_ann) { return bt::host_sharpe(s1, s2, n, sqrt_ann); }
int64_t n_ret(const bt_fold& f) { return bt::fold_ret_bars(f); }

bt_fold empty_fold(int32_t first_bar) {
    bt_fold f;
    memset(&f, 0, sizeof f);
    f.first_bar = first_bar;
    return f;
}

// One row's steps from its fold records row[p * K + k].
void row_steps(const bt_fold* row, int32_t P, int32_t K, int32_t train, int32_t id, double sqrt_ann,
               bt_wf_step* out) {
    const int32_t j0 = train > 1 ? train : 1;
    for (int32_t j = j0; j < K; ++j) {
        const int32_t f0 = train == 0 ? 0 : j - train;
        int64_t n = 0;
        for (int32_t k = f0; k < j; ++k) n += n_ret(row[k]);
        bt_wf_step s;
        memset(&s, 0, sizeof s);
        s.sym = id;
        s.fold = j;
        s.param = -1;
        s.oos = empty_fold(row[j].first_bar);
        if (n > 0 && row[j].n_bars > 0) {
            double best = 0.0;
            for (int32_t p = 0; p < P; ++p) {
                i128 s1 = 0, s2 = 0;
                for (int32_t k = f0; k < j; ++k) {
                    const bt_fold& f = row[(size_t)p * (size_t)K + (size_t)k];
                    s1 += wide_join(f.s1_lo, f.s1_hi);
                    s2 += wide_join(f.s2_lo, f.s2_hi);
                }
                const double sh = sharpe_of(s1, s2, n, sqrt_ann);
                if (s.param < 0 || sharpe_key(sh) > sharpe_key(best)) {  // ties stay with the lower p
                    best = sh;
                    s.param = p;
                }
            }
            s.train_sharpe = best;
            s.oos = row[(size_t)s.param * (size_t)K + (size_t)j];
        }
        out[j - j0] = s;
    }
}

}  // namespace

namespace bt {

void walkfwd_totals(int32_t S, int32_t n_steps, const bt_wf_step* steps, double sqrt_ann, bt_fold* total) {
    for (int32_t s = 0; s < S; ++s) {
        bt_fold t = empty_fold(0);
        i128 s1 = 0, s2 = 0;
        int64_t n = 0;
        bool any = false;
        for (int32_t i = 0; i < n_steps; ++i) {
            const bt_wf_step& st = steps[(size_t)s * (size_t)n_steps + (size_t)i];
            if (st.param < 0) continue;
            const bt_fold& f = st.oos;
            if (!any) t.first_bar = f.first_bar;
            any = true;
            t.n_bars += f.n_bars;
            t.n_trades += f.n_trades;
            t.pnl += f.pnl;
            t.exposure += f.exposure;
            if (f.mdd > t.mdd) t.mdd = f.mdd;
            s1 += wide_join(f.s1_lo, f.s1_hi);
            s2 += wide_join(f.s2_lo, f.s2_hi);
            n += n_ret(f);
        }
        wide_split(s1, t.s1_lo, t.s1_hi);
        wide_split(s2, t.s2_lo, t.s2_hi);
        t.sharpe = sharpe_of(s1, s2, n, sqrt_ann);
        total[s] = t;
    }
}

}  // namespace bt

extern "C" {

int32_t bt_walk_forward_host(int32_t S, int32_t P, int32_t K, int32_t train, const bt_fold* folds,
                             const int32_t* sym_ids, int64_t annualization, bt_wf_step* steps,
                             bt_fold* total) {
    const char* fn = "bt_walk_forward_host";
    try {
        if (S < 0) return refuse(fn, "S = " + std::to_string(S) + " is negative");
        if (P < 1) return refuse(fn, "P = " + std::to_string(P) + " is below 1");
        if (!steps && !total) return refuse(fn, "steps and total are both NULL");
        const std::string why = bt::walkfwd_refusal(K, nullptr, train, false, steps != nullptr, total != nullptr, S, P);
        if (!why.empty()) return refuse(fn, why);
        if (annualization <= 0)
            return refuse(fn, "annualization = " + std::to_string(annualization) + " is not positive");
        if (S > 0 && (!folds || !sym_ids)) return refuse(fn, "folds and sym_ids are required");
        const double sqrt_ann = std::sqrt((double)annualization);
        const int32_t n_steps = bt::walkfwd_steps(K, train);
        std::vector<bt_wf_step> own;
        bt_wf_step* st = steps;
        if (!st) {
            own.resize((size_t)S * (size_t)n_steps);
            st = own.data();
        }
        for (int32_t s = 0; s < S; ++s)
            row_steps(folds + (size_t)s * (size_t)P * (size_t)K, P, K, train, sym_ids[s], sqrt_ann,
                      st + (size_t)s * (size_t)n_steps);
        if (total) bt::walkfwd_totals(S, n_steps, st, sqrt_ann, total);
        return 0;
    } catch (const std::exception& x) {
        return refuse(fn, std::string("exception: ") + x.what());
    }
}

}  // extern "C"
