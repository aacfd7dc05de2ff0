// tstats.h — host side of the per-lane trade statistics (docs/tradestats_spec.md): the record
// layouts, the argument rules of bt_trade_stats and what tstats.cpp shares with analysis.cpp. No HIP
// type: tstats.cpp builds with a plain host compiler (tests/asan).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "host_common.h"

// bt_tstats: four int32 counts, two long counts, two streaks, four hold / bar words (48 bytes),
// then ten 8-byte words: gross_win, gross_loss, max_win, max_loss, sq (lo, hi), mdd, the two bars,
// the two under-water counts, hash.
static_assert(sizeof(bt_tstats) == 128, "bt_tstats layout");
static_assert(offsetof(bt_tstats, n_long) == 16 && offsetof(bt_tstats, hold_sum) == 32 &&
                  offsetof(bt_tstats, gross_win) == 48 && offsetof(bt_tstats, sq_lo) == 80 &&
                  offsetof(bt_tstats, mdd) == 96 && offsetof(bt_tstats, mdd_bar) == 104 &&
                  offsetof(bt_tstats, underwater_bars) == 112 && offsetof(bt_tstats, hash) == 120,
              "bt_tstats layout");
// bt_tstats_agg: six int32 (24 bytes), nine int64 sums, three int64 maxima, sq (lo, hi).
static_assert(sizeof(bt_tstats_agg) == 136, "bt_tstats_agg layout");
static_assert(offsetof(bt_tstats_agg, n_trades) == 24 && offsetof(bt_tstats_agg, max_win) == 96 &&
                  offsetof(bt_tstats_agg, sq_lo) == 120,
              "bt_tstats_agg layout");

namespace bt {

// Why the arguments of bt_trade_stats are refused ("" = accepted), in the order the call checks
// them: the dataset, n, the mode (list mode with lanes, all-lanes mode without) and its outputs.
std::string tstats_refusal(bool have_dataset, int64_t n, bool have_lanes, bool have_out, bool have_agg);

// One row's P records against the staging budget (rows_per_chunk == 0 of plan_tstats).
std::string tstats_budget_refusal(int64_t P, int64_t budget);

}  // namespace bt
