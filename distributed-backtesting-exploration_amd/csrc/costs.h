// costs.h — host side of the net-of-costs call (docs/costs_spec.md): the record layouts, the
// argument rules of bt_costs and what costs.cpp shares with analysis.cpp. No HIP type: costs.cpp
// builds with a plain host compiler (tests/asan).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "host_common.h"

// bt_cost_rec: four int32 counts, the drawdown bar and the under-water count (24 bytes), then eight
// 8-byte words: pnl, fees, turnover, mdd, win_sum, loss_sum, s2 (lo, hi).
static_assert(sizeof(bt_cost_rec) == 88, "bt_cost_rec layout");
static_assert(offsetof(bt_cost_rec, n_trades) == 0 && offsetof(bt_cost_rec, n_win) == 4 &&
                  offsetof(bt_cost_rec, n_loss) == 8 && offsetof(bt_cost_rec, n_bars) == 12 &&
                  offsetof(bt_cost_rec, mdd_bar) == 16 && offsetof(bt_cost_rec, underwater_bars) == 20 &&
                  offsetof(bt_cost_rec, pnl) == 24 && offsetof(bt_cost_rec, fees) == 32 &&
                  offsetof(bt_cost_rec, turnover) == 40 && offsetof(bt_cost_rec, mdd) == 48 &&
                  offsetof(bt_cost_rec, win_sum) == 56 && offsetof(bt_cost_rec, loss_sum) == 64 &&
                  offsetof(bt_cost_rec, s2_lo) == 72 && offsetof(bt_cost_rec, s2_hi) == 80,
              "bt_cost_rec layout");
// bt_cost_agg: four int32 (16 bytes), three int64 sums, one int64 maximum.
static_assert(sizeof(bt_cost_agg) == 48, "bt_cost_agg layout");
static_assert(offsetof(bt_cost_agg, n_sym) == 0 && offsetof(bt_cost_agg, n_traded) == 4 &&
                  offsetof(bt_cost_agg, n_profit) == 8 && offsetof(bt_cost_agg, pad) == 12 &&
                  offsetof(bt_cost_agg, trades) == 16 && offsetof(bt_cost_agg, pnl) == 24 &&
                  offsetof(bt_cost_agg, fees) == 32 && offsetof(bt_cost_agg, mdd_max) == 40,
              "bt_cost_agg layout");

namespace bt {

// Why the arguments of bt_costs are refused ("" = accepted), in the order the call checks them: the
// dataset, C, the levels (each level's range, the level named), n, the mode (list mode with lanes,
// all-lanes mode without) and its outputs. `levels`: C pairs (fixed, bps), or nullptr.
std::string costs_refusal(bool have_dataset, int64_t C, const int32_t* levels, int64_t n, bool have_lanes,
                          bool have_out, bool have_agg);

// C and the levels alone: what bt_costs_host checks of them too.
std::string cost_levels_refusal(int64_t C, const int32_t* levels);

// One row's P * C records against the staging budget (per_chunk == 0 of plan_costs).
std::string costs_budget_refusal(int64_t P, int64_t C, int64_t budget);

}  // namespace bt
