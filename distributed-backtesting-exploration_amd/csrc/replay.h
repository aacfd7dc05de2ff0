// replay.h — host side of the lane replay (bt_replay): the rules its arguments must meet and the
// resolution of the requested lanes against the dataset, shared by replay.cpp and analysis.cpp.
// No HIP call: replay.cpp builds host-only (tests/plan/replay_plan_driver.cpp).
#pragma once
#include <unordered_map>
#include <vector>

#include "internal.h"

namespace bt {

// Why the arguments of a replay are refused ("" = accepted), in the order the call checks them:
// the dataset, n, trade_cap against the trades buffer and, for n > 0, the lanes and summaries.
std::string replay_refusal(bool have_dataset, int64_t n, int64_t trade_cap, bool have_trades,
                           bool have_lanes, bool have_sum);

// Global symbol id -> dataset row; the first row of a repeated id wins (bt_replay, bt_portfolio).
std::unordered_map<int32_t, int32_t> symbol_rows(const SymDesc* syms, size_t n_sym);

// The n requests against the dataset's rows: global symbol id -> the first row with that id, the
// param against [0, P), and with curves the stride against W, the longest requested symbol.
// Fills `req` and `W`; returns "" or the refusal, which names the value and the lane.
std::string replay_resolve(const SymDesc* syms, size_t n_sym, int32_t P, int32_t n, const bt_lane* lanes,
                           bool curves, int64_t stride, std::vector<ReplayLane>& req, int32_t& W);

}  // namespace bt
