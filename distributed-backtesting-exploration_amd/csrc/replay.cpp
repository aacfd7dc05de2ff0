// replay.cpp — the host rules of bt_replay (replay.h). Pure functions: no HIP call, no device state.
#include "replay.h"

#include <algorithm>

namespace bt {

std::string replay_refusal(bool have_dataset, int64_t n, int64_t trade_cap, bool have_trades,
                           bool have_lanes, bool have_sum) {
    if (!have_dataset) return "no dataset loaded";
    if (n < 0 || n > BT_REPLAY_MAX)
        return "n = " + std::to_string(n) + " outside [0, " + std::to_string(BT_REPLAY_MAX) + "]";
    if (trade_cap < 0) return "trade_cap = " + std::to_string(trade_cap) + " is negative";
    if (have_trades && trade_cap == 0) return "trades given with trade_cap = 0";
    if (!have_trades && trade_cap > 0)
        return "trade_cap = " + std::to_string(trade_cap) + " without a trades buffer";
    if (n > 0 && (!have_lanes || !have_sum)) return "lanes and sum are required";
    return "";
}

std::unordered_map<int32_t, int32_t> symbol_rows(const SymDesc* syms, size_t n_sym) {
    std::unordered_map<int32_t, int32_t> row;
    row.reserve(n_sym);
    for (size_t s = 0; s < n_sym; ++s) row.emplace(syms[s].id, (int32_t)s);
    return row;
}

std::string replay_resolve(const SymDesc* syms, size_t n_sym, int32_t P, int32_t n, const bt_lane* lanes,
                           bool curves, int64_t stride, std::vector<ReplayLane>& req, int32_t& W) {
    const std::unordered_map<int32_t, int32_t> row = symbol_rows(syms, n_sym);
    req.resize((size_t)std::max(n, 0));
    W = 0;
    for (int32_t i = 0; i < n; ++i) {
        const auto it = row.find(lanes[i].sym);
        if (it == row.end())
            return "unknown symbol id " + std::to_string(lanes[i].sym) + " (lane " + std::to_string(i) + ")";
        if (lanes[i].param < 0 || lanes[i].param >= P)
            return "param " + std::to_string(lanes[i].param) + " outside [0, " + std::to_string(P) +
                   ") (lane " + std::to_string(i) + ")";
        const SymDesc& sd = syms[(size_t)it->second];
        req[i] = ReplayLane{sd.off, sd.bars, lanes[i].param};
        W = std::max(W, sd.bars);
    }
    if (curves && stride < W)
        return "stride = " + std::to_string(stride) + " shorter than the longest requested symbol (" +
               std::to_string(W) + " bars)";
    return "";
}

}  // namespace bt
