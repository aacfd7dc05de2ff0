// cscv.h — host side of the probability of backtest overfitting (docs/cscv_spec.md): what cscv.cpp
// shares with analysis.cpp and plan.cpp. No HIP type: cscv.cpp builds with a plain host compiler
// (tests/asan).
#pragma once
#include <stdint.h>

#include <string>

#include "host_common.h"

static_assert(sizeof(bt_cscv_group) == 32, "bt_cscv_group layout");
static_assert(sizeof(bt_cscv_pick) == 24, "bt_cscv_pick layout");

namespace bt {

constexpr int64_t kCscvPicksMax = 1LL << 22;       // pick records a call returns
constexpr int kCscvSumBits = 120;                  // |s1|, s2 of a staged record lie below 2^120

// C = binom(K, K/2) of an even K in [2, BT_CSCV_MAX_FOLDS] (184,756 at K = 20).
inline int64_t cscv_combos(int32_t K) {
    int64_t c = 1;
    for (int32_t i = 1; i <= K / 2; ++i) c = c * (K / 2 + i) / i;   // exact: a binomial at every step
    return c;
}

// Why a call is refused ("" = accepted): K, the bounds (K + 1 values, checked as bt_walk_forward
// checks them when not NULL), the outputs asked for, and G*C against kCscvPicksMax with picks.
std::string cscv_refusal(int64_t K, const int32_t* bounds, bool want_groups, bool want_hist, bool want_picks, int64_t G);

// Why staged fold records folds[G][P][K] are refused ("" = accepted): the shape, lanes of a group
// that disagree in a fold's bars, bar counts out of range and sums outside the domain.
std::string cscv_folds_refusal(int64_t G, int64_t P, int32_t K, const bt_fold* folds);

}  // namespace bt
