// portfolio.h — host side of the portfolio of chosen lanes (bt_portfolio; docs/portfolio_spec.md):
// the rules its arguments must meet, the resolution of the entries against the dataset, and the
// scalar finish (equity and summary from the per-bar rows), shared by portfolio.cpp and
// analysis.cpp. No HIP call: portfolio.cpp builds host-only (tests/asan/portfolio_driver.cpp).
#pragma once
#include <vector>

#include "internal.h"

static_assert(sizeof(bt_pf_lane) == 16, "bt_pf_lane layout");
static_assert(sizeof(bt_pf_summary) == 80, "bt_pf_summary layout");

namespace bt {

constexpr int32_t kPortfolioMaxT = 1 << 22;            // bars of the output rows (the longest symbol)
constexpr int64_t kPortfolioMaxWindowBars = 1LL << 30;  // window bars of all entries together

// Why the arguments of a portfolio call are refused ("" = accepted), in the order the call checks
// them: the dataset, n, the lanes, T and the outputs.
std::string portfolio_refusal(bool have_dataset, int64_t n, bool have_lanes, int64_t T, bool any_output);

// One entry's window against its symbol's bars and T: "" or the refusal, which names the value and
// the entry. Fills the clipped window [from, to) (to == from when it is empty).
std::string portfolio_window(int64_t i, int32_t from_bar, int32_t to_bar, int32_t bars, int32_t T,
                             int32_t& from, int32_t& to);

// What the entries come to once resolved: the device descriptors of those with a non-empty window,
// in request order, and the summary's n_lanes, lo and hi (0, 0, 0 without one).
struct PfResolved {
    std::vector<PfLane> req;
    int32_t n_lanes = 0, lo = 0, hi = 0;
    int64_t window_bars = 0;
    // one more non-empty window; "" or the refusal once the total passes kPortfolioMaxWindowBars
    std::string count(int32_t from, int32_t to);
};
// The n entries against the dataset's rows: global symbol id -> the first row with that id
// (replay.h symbol_rows), the param against [0, P), the window rules above.
std::string portfolio_resolve(const SymDesc* syms, size_t n_sym, int32_t P, int32_t n, const bt_pf_lane* lanes,
                              int32_t T, PfResolved& out);

// equity[T] (may be NULL) and the summary from the per-bar rows, as docs/portfolio_spec.md §3/§4
// define them, with __int128 sums: what bt_portfolio_host and bt_portfolio_merge end with.
void portfolio_finish_host(int32_t T, int32_t n_lanes, int32_t lo, int32_t hi, const int64_t* pnl,
                           const int32_t* n_long, const int32_t* n_short, double sqrt_ann, int64_t* equity,
                           bt_pf_summary* sum);

}  // namespace bt
