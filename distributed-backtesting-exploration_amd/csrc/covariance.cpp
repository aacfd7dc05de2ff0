// covariance.cpp — the host rules of bt_covariance and bt_gram_of (covariance.h) and the scalar
// restatement of what k_gram.hip computes: bt_covariance_host, from per-lane equity curves as
// bt_replay returns them. Written from docs/covariance_spec.md with the compiler's __int128: plain
// integer products, no 16-bit split and no floating point, so that it shares nothing with the
// kernels and the two check each other. Pure code: no HIP call, no device state.
#include "covariance.h"

#include <algorithm>
#include <exception>
#include <vector>

namespace bt {

std::string covariance_refusal(bool have_dataset, int64_t n, bool have_lanes, int32_t from_bar, int32_t to_bar,
                               bool any_output) {
    if (!have_dataset) return "no dataset loaded";
    if (n < 0 || n > BT_COV_MAX)
        return "n = " + std::to_string(n) + " outside [0, " + std::to_string(BT_COV_MAX) + "]";
    if (n > 0 && !have_lanes) return "lanes are required";
    if (from_bar < 0) return "from_bar = " + std::to_string(from_bar) + " is negative";
    if (to_bar < from_bar)
        return "to_bar = " + std::to_string(to_bar) + " is below from_bar = " + std::to_string(from_bar);
    if (!any_output) return "gram, sums and T are all NULL";
    return "";
}

std::string covariance_window(int32_t from_bar, int32_t to_bar, int32_t b_max, int32_t& T) {
    const int64_t t = (int64_t)std::min(to_bar, b_max) - from_bar;
    T = (int32_t)std::max<int64_t>(0, std::min<int64_t>(t, INT32_MAX));
    if (T > kGramMaxT)
        return "T = " + std::to_string(T) + " bars of the window [" + std::to_string(from_bar) + ", " +
               std::to_string(std::min(to_bar, b_max)) + ") above 2^22";
    return "";
}

std::string gram_of_refusal(int64_t n, int64_t T, bool have_d, bool any_output) {
    if (n < 0 || n > BT_COV_MAX)
        return "n = " + std::to_string(n) + " outside [0, " + std::to_string(BT_COV_MAX) + "]";
    if (T < 0 || T > kGramMaxT)
        return "T = " + std::to_string(T) + " outside [0, " + std::to_string(kGramMaxT) + "]";
    if (n > 0 && T > 0 && !have_d) return "d is required";
    if (!any_output) return "gram and sums are both NULL";
    return "";
}

std::string gram_staging_refusal(size_t staging_bytes, size_t max_bytes, int64_t n, int64_t T) {
    if (staging_bytes <= max_bytes) return "";
    return "n = " + std::to_string(n) + " lanes over T = " + std::to_string(T) + " bars need " +
           std::to_string(staging_bytes) + " bytes of device staging, above " + std::to_string(max_bytes);
}

}  // namespace bt

using bt::refuse;

extern "C" {

int32_t bt_covariance_host(int32_t n, const int64_t* equity, const int32_t* n_bars, int64_t stride,
                           int32_t from_bar, int32_t to_bar, bt_wide* gram, int64_t* sums, int32_t* T_out) {
    const char* fn = "bt_covariance_host";
    try {
        std::string why = bt::covariance_refusal(true, n, true, from_bar, to_bar, gram || sums || T_out);
        int32_t b_max = 0, T = 0;
        if (why.empty()) why = bt::curves_refusal(n, equity && n_bars, "equity and n_bars", n_bars, stride, "lane", b_max);
        if (why.empty()) why = bt::covariance_window(from_bar, to_bar, b_max, T);
        if (!why.empty()) return refuse(fn, why);
        const std::vector<int64_t> d = bt::curve_increments(n, equity, n_bars, stride, from_bar, T, sums);
        if (gram)
            for (int32_t i = 0; i < n; ++i)
                for (int32_t j = i; j < n; ++j) {
                    const int64_t* a = d.data() + (size_t)i * (size_t)T;
                    const int64_t* b = d.data() + (size_t)j * (size_t)T;
                    __int128 v = 0;
                    for (int32_t t = 0; t < T; ++t) v += (__int128)a[t] * (__int128)b[t];
                    const bt_wide x = bt::wide_rec(v);
                    gram[(size_t)i * (size_t)n + (size_t)j] = x;
                    gram[(size_t)j * (size_t)n + (size_t)i] = x;
                }
        if (T_out) *T_out = T;
        return 0;
    } catch (const std::exception& x) {
        return refuse(fn, std::string("exception: ") + x.what());
    }
}

}  // extern "C"
