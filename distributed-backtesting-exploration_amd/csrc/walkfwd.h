// walkfwd.h — host side of the walk-forward evaluation (docs/walkforward_spec.md): what walkfwd.cpp
// shares with analysis.cpp. No HIP type: walkfwd.cpp builds with a plain host compiler (tests/asan).
#pragma once
#include <stdint.h>

#include <string>

#include "host_common.h"

static_assert(sizeof(bt_fold) == 80, "bt_fold layout");
static_assert(sizeof(bt_wf_step) == 104, "bt_wf_step layout");

namespace bt {

constexpr int64_t kWalkfwdFoldsMax = 1LL << 22;    // fold records bt_walk_forward returns

// Why a walk-forward call is refused ("" = accepted): K, the bounds (K + 1 values, checked when
// not NULL), train, the outputs asked for, and S*P*K against kWalkfwdFoldsMax when the fold
// records are among them.
std::string walkfwd_refusal(int64_t K, const int32_t* bounds, int64_t train, bool want_folds,
                            bool want_steps, bool want_total, int64_t S, int64_t P);

// Steps j = max(train, 1) .. K - 1 of a call.
inline int32_t walkfwd_steps(int32_t K, int32_t train) { return K - (train > 1 ? train : 1); }

// total[s] from the n_steps steps of each of S rows (spec "per-row total").
void walkfwd_totals(int32_t S, int32_t n_steps, const bt_wf_step* steps, double sqrt_ann, bt_fold* total);

}  // namespace bt
