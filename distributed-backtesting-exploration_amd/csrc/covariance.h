// covariance.h — host side of the covariance of chosen lanes (bt_covariance, bt_gram_of;
// docs/covariance_spec.md): the rules their arguments must meet, shared by covariance.cpp and
// analysis.cpp. No HIP call: covariance.cpp builds host-only (tests/asan/gram_driver.cpp).
#pragma once
#include "internal.h"

static_assert(sizeof(bt_wide) == 16, "bt_wide layout");

namespace bt {

constexpr int32_t kGramMaxT = 1 << 22;   // bars of a window: the exactness bound of k_gram.hip

// Why the arguments of bt_covariance are refused ("" = accepted), in the order the call checks
// them: the dataset, n, the lanes, the window's ends and the outputs.
std::string covariance_refusal(bool have_dataset, int64_t n, bool have_lanes, int32_t from_bar, int32_t to_bar,
                               bool any_output);

// The window against B_max, the bars of the longest requested symbol: fills T = max(0,
// min(to_bar, B_max) - from_bar); "" or the refusal of a T above kGramMaxT.
std::string covariance_window(int32_t from_bar, int32_t to_bar, int32_t b_max, int32_t& T);

// Why the arguments of bt_gram_of are refused: n, T, the matrix and the outputs.
std::string gram_of_refusal(int64_t n, int64_t T, bool have_d, bool any_output);

// The old name of increments_domain_refusal (host_common.h), kept like internal.h's ReplayLane:
// tests/asan/gram_driver.cpp builds with it.
inline std::string gram_domain_refusal(int64_t n, int64_t T, const int32_t* d) {
    return increments_domain_refusal(n, T, d);
}

// "" or the refusal of a plan whose staging exceeds `max_bytes` (plan.h kGramStagingMax).
std::string gram_staging_refusal(size_t staging_bytes, size_t max_bytes, int64_t n, int64_t T);

}  // namespace bt
