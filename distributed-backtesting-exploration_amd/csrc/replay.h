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

// The n requests of a call against the dataset's rows: global symbol id -> the first row with that
// id, the param against [0, P); each(i, LaneRef) then takes the request and returns "" or a refusal
// of its own. Returns "" or the first refusal, which names the value and the request as
// "(`noun` i)" ("lane", "entry"). The text is built out of line: a book has tens of thousands of
// entries and a call of a millisecond.
std::string lane_refusal(bool unknown, int32_t sym, int32_t param, int32_t P, const char* noun, int64_t i);
template <class Lane, class Each>
std::string resolve_lanes(const SymDesc* syms, size_t n_sym, int32_t P, int32_t n, const Lane* lanes,
                          const char* noun, Each&& each) {
    const std::unordered_map<int32_t, int32_t> row = symbol_rows(syms, n_sym);
    for (int32_t i = 0; i < n; ++i) {
        const auto it = row.find(lanes[i].sym);
        if (it == row.end() || lanes[i].param < 0 || lanes[i].param >= P)
            return lane_refusal(it == row.end(), lanes[i].sym, lanes[i].param, P, noun, i);
        const SymDesc& sd = syms[(size_t)it->second];
        std::string why = each(i, LaneRef{sd.off, sd.bars, lanes[i].param});
        if (!why.empty()) return why;
    }
    return "";
}

// The lanes of bt_replay and bt_covariance through resolve_lanes: fills `req` and `W`, the longest
// requested symbol.
std::string lanes_resolve(const SymDesc* syms, size_t n_sym, int32_t P, int32_t n, const bt_lane* lanes,
                          std::vector<LaneRef>& req, int32_t& W);

// lanes_resolve and, with curves, the stride against W.
std::string replay_resolve(const SymDesc* syms, size_t n_sym, int32_t P, int32_t n, const bt_lane* lanes,
                           bool curves, int64_t stride, std::vector<LaneRef>& req, int32_t& W);

}  // namespace bt
