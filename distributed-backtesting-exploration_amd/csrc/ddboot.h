// ddboot.h — host side of the drawdown bootstrap (docs/drawdown_spec.md): the record layout, the
// argument rules of bt_drawdown_boot / bt_drawdown_boot_of and what ddboot.cpp shares with
// analysis.cpp. The window, the draws and the increments' domain are the reality check's
// (bootstrap.h, host_common.h). No HIP type: ddboot.cpp builds with a plain host compiler
// (tests/asan).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "bootstrap.h"

static_assert(sizeof(bt_dd_lane) == 72, "bt_dd_lane layout");
static_assert(offsetof(bt_dd_lane, sum) == 0 && offsetof(bt_dd_lane, mdd) == 8 && offsetof(bt_dd_lane, n_ge) == 16 &&
                  offsetof(bt_dd_lane, min_star) == 24 && offsetof(bt_dd_lane, max_star) == 32 &&
                  offsetof(bt_dd_lane, m1) == 40 && offsetof(bt_dd_lane, m2) == 56,
              "bt_dd_lane layout");

namespace bt {

constexpr int32_t kDdPpmMax = 1000000;

// What a call was given, for the rules below. `staged`: bt_drawdown_boot_of (no dataset, no window).
struct DdCall {
    bool have_engine, have_dataset, staged;
    bool have_lanes;                 // list mode; a staged call: d given
    int64_t n;
    int64_t from_bar;
    int64_t B, L;
    int64_t Q;
    const int32_t* alpha_ppm;        // [Q] or NULL
    int64_t R;
    const int64_t* limits;           // [R] or NULL
    bool have_rec, have_q, have_reach, have_raw;
};

// Q and the levels, R and the limits alone ("" = accepted): what the three calls share.
std::string dd_levels_refusal(int64_t Q, const int32_t* alpha_ppm, int64_t R, const int64_t* limits);

// Why the arguments are refused ("" = accepted), in the order the call checks them: the engine, the
// dataset, the mode and n, from_bar, B, L, the levels, the limits, the outputs. The window's T is
// checked by boot_window once the rows are known.
std::string dd_refusal(const DdCall& c);

// The smallest staging the call can run in against the budget, and a row (prefix row and block
// tables) against the LDS a workgroup may take (bt_set_ddboot_row mode 1).
std::string dd_budget_refusal(size_t need_bytes, size_t budget);
std::string dd_row_refusal(int64_t T, size_t row_bytes, size_t limit_bytes);

// Rank of level alpha_ppm among B values: ceil(B * alpha_ppm / 10^6), in [1, B].
inline int64_t dd_rank(int64_t B, int64_t alpha_ppm) { return (B * alpha_ppm + kDdPpmMax - 1) / kDdPpmMax; }

}  // namespace bt
