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

std::string lane_refusal(bool unknown, int32_t sym, int32_t param, int32_t P, const char* noun, int64_t i) {
    const std::string which = std::string(" (") + noun + " " + std::to_string(i) + ")";
    if (unknown) return "unknown symbol id " + std::to_string(sym) + which;
    return "param " + std::to_string(param) + " outside [0, " + std::to_string(P) + ")" + which;
}

std::string lanes_resolve(const SymDesc* syms, size_t n_sym, int32_t P, int32_t n, const bt_lane* lanes,
                          std::vector<LaneRef>& req, int32_t& W) {
    req.resize((size_t)std::max(n, 0));
    W = 0;
    return resolve_lanes(syms, n_sym, P, n, lanes, "lane", [&](int32_t i, const LaneRef& ref) {
        req[i] = ref;
        W = std::max(W, ref.bars);
        return std::string();
    });
}

std::string replay_resolve(const SymDesc* syms, size_t n_sym, int32_t P, int32_t n, const bt_lane* lanes,
                           bool curves, int64_t stride, std::vector<LaneRef>& req, int32_t& W) {
    const std::string why = lanes_resolve(syms, n_sym, P, n, lanes, req, W);
    if (!why.empty()) return why;
    if (curves && stride < W)
        return "stride = " + std::to_string(stride) + " shorter than the longest requested symbol (" +
               std::to_string(W) + " bars)";
    return "";
}

}  // namespace bt
