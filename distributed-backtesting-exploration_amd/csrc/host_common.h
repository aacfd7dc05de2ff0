// host_common.h — what the host rule files of the analysis calls (surface.cpp, walkfwd.cpp,
// cscv.cpp, tstats.cpp, costs.cpp, tail.cpp, bootstrap.cpp, portfolio.cpp, covariance.cpp) and analysis.cpp share: the
// one error path of a HIP-free entry point, the int128 word helpers, the host Sharpe of fold
// sums and the rules of replayed curves and staged increments. No HIP include: a plain host compiler builds it (the drivers under
// tests/asan); internal.h includes it, so the word helpers serve the kernels too.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/bt.h"

#ifdef __HIPCC__
#define BT_HD __host__ __device__
#else
#define BT_HD
#endif

namespace bt {

typedef __int128 i128;

void set_last_error(const std::string& s);  // bt_last_error() of this thread (engine.cpp)

// The refusal of a HIP-free entry point: `fn: why` becomes bt_last_error(), the call returns -1.
inline int32_t refuse(const char* fn, const std::string& why) {
    set_last_error(std::string(fn) + ": " + why);
    return -1;
}

// An int128 as the (lo, hi) words of the ABI's records, and back.
BT_HD inline i128 wide_join(uint64_t lo, int64_t hi) {
    return (i128)(((unsigned __int128)(uint64_t)hi << 64) | lo);
}
BT_HD inline uint64_t wide_lo(i128 x) { return (uint64_t)x; }
BT_HD inline int64_t wide_hi(i128 x) { return (int64_t)(x >> 64); }
BT_HD inline void wide_split(i128 x, uint64_t& lo, int64_t& hi) { lo = wide_lo(x), hi = wide_hi(x); }
BT_HD inline bt_wide wide_rec(i128 x) { return bt_wide{wide_lo(x), wide_hi(x)}; }

// The engine's orderable Sharpe (oracle spec §5) on the host: the double's bits, monotone as an
// unsigned integer.
inline uint64_t host_sharpe_key(double x) {
    uint64_t u;
    memcpy(&u, &x, sizeof u);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ULL);
}

// walkforward_spec §4's Sharpe of the sums over n return bars (0 when there are none), with the
// compiler's int128: the conversion of the sums rounds to nearest, ties to even.
inline double host_sharpe(i128 s1, i128 s2, int64_t n, double sqrt_ann) {
    if (n < 1) return 0.0;
    const double nn = (double)n;
    const double m = std::ldexp((double)s1, -56) / nn;
    const double mm = m * m;
    const double v = std::ldexp((double)s2, -56) / nn - mm;
    return v > 0 ? (m / std::sqrt(v)) * sqrt_ann : 0.0;
}

// Return bars of a fold record: its bars but bar 0.
inline int64_t fold_ret_bars(const bt_fold& f) {
    return (int64_t)f.n_bars - (f.first_bar == 0 && f.n_bars > 0 ? 1 : 0);
}

// d[n][T] of a staged call (bt_gram_of, bt_bootstrap_of) against |d| < 2^31.
inline std::string increments_domain_refusal(int64_t n, int64_t T, const int32_t* d) {
    const int64_t cells = n * T;
    for (int64_t k = 0; k < cells; ++k)
        if (d[k] == INT32_MIN)
            return "d[" + std::to_string(k / T) + "][" + std::to_string(k % T) + "] = " + std::to_string(INT32_MIN) +
                   " outside the domain |d| < 2^31";
    return "";
}

// The curves of n lanes as bt_replay returns them, row i with n_bars[i] <= stride values, as the
// *_host calls take them: `have`: every array of `names` was given; `noun` names a row in the
// refusal ("lane", "entry"). "" and b_max, the longest row, or the refusal.
inline std::string curves_refusal(int32_t n, bool have, const char* names, const int32_t* n_bars, int64_t stride,
                                  const char* noun, int32_t& b_max) {
    b_max = 0;
    if (n > 0 && !have) return std::string(names) + " are required";
    if (n > 0 && stride < 0) return "stride = " + std::to_string(stride) + " is negative";
    for (int32_t i = 0; i < n; ++i) {
        if (n_bars[i] < 0 || n_bars[i] > stride)
            return "n_bars = " + std::to_string(n_bars[i]) + " outside [0, stride = " + std::to_string(stride) + "] (" +
                   noun + " " + std::to_string(i) + ")";
        b_max = std::max(b_max, n_bars[i]);
    }
    return "";
}

// Such curves as increments over the window [from_bar, from_bar + T):
// d[i][k] = E_i[from_bar + k] - E_i[from_bar + k - 1] with E[-1] = 0, zero past the lane's own
// bars, and, when asked for, every row's sum.
inline std::vector<int64_t> curve_increments(int32_t n, const int64_t* equity, const int32_t* n_bars, int64_t stride,
                                             int32_t from_bar, int32_t T, int64_t* sums) {
    std::vector<int64_t> d((size_t)n * (size_t)T, 0);
    for (int32_t i = 0; i < n; ++i) {
        const int64_t* E = equity + (size_t)i * (size_t)stride;
        const int64_t end = std::min<int64_t>((int64_t)from_bar + T, n_bars[i]);
        int64_t s = 0;
        for (int64_t t = from_bar; t < end; ++t) {
            const int64_t x = E[t] - (t > 0 ? E[t - 1] : 0);
            d[(size_t)i * (size_t)T + (size_t)(t - from_bar)] = x;
            s += x;
        }
        if (sums) sums[i] = s;
    }
    return d;
}

}  // namespace bt
