// tail.h — host side of the tail-risk call (docs/tail_spec.md): the record layouts, the argument
// rules of bt_tail and bt_tail_of and what tail.cpp shares with analysis.cpp. No HIP type: tail.cpp
// builds with a plain host compiler (tests/asan).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "host_common.h"

// bt_tail_rec: six int32 (24 bytes), four int64, three int128 as (lo, hi) words, one 192-bit sum.
static_assert(sizeof(bt_tail_rec) == 128, "bt_tail_rec layout");
static_assert(offsetof(bt_tail_rec, n) == 0 && offsetof(bt_tail_rec, n_window) == 4 &&
                  offsetof(bt_tail_rec, n_pos) == 8 && offsetof(bt_tail_rec, n_neg) == 12 &&
                  offsetof(bt_tail_rec, min_bar) == 16 && offsetof(bt_tail_rec, max_bar) == 20 &&
                  offsetof(bt_tail_rec, min_d) == 24 && offsetof(bt_tail_rec, max_d) == 32 &&
                  offsetof(bt_tail_rec, s1) == 40 && offsetof(bt_tail_rec, s1_neg) == 48 &&
                  offsetof(bt_tail_rec, s2) == 56 && offsetof(bt_tail_rec, s2_neg) == 72 &&
                  offsetof(bt_tail_rec, s3) == 88 && offsetof(bt_tail_rec, s4) == 104,
              "bt_tail_rec layout");
static_assert(sizeof(bt_tail_q) == 24, "bt_tail_q layout");
static_assert(offsetof(bt_tail_q, var) == 0 && offsetof(bt_tail_q, es_sum) == 8 && offsetof(bt_tail_q, k) == 16 &&
                  offsetof(bt_tail_q, n_lt) == 20,
              "bt_tail_q layout");

namespace bt {

// Q and the levels alone ("" = accepted): what bt_tail, bt_tail_of and bt_tail_host share.
std::string tail_levels_refusal(int64_t Q, const int32_t* alpha_ppm);

// Why the arguments of bt_tail are refused ("" = accepted), in the order the call checks them: the
// dataset, n and the mode of the request (list mode with lanes, all-lanes mode without), Q and the
// levels (the level named), the counting mode, the window, the outputs and the longest dataset row.
std::string tail_refusal(bool have_dataset, int64_t n, bool have_lanes, int64_t from_bar, int64_t to_bar, int64_t mode,
                         int64_t Q, const int32_t* alpha_ppm, bool have_recs, bool have_q, int64_t max_bars);

// ... and of bt_tail_of, before its increments are read (increments_domain_refusal).
std::string tail_of_refusal(int64_t n, int64_t T, bool have_d, int64_t Q, const int32_t* alpha_ppm, bool have_recs,
                            bool have_q);

// The window [from_bar, to_bar) against rows of at most `longest` bars: the most bars a lane can
// count, min(to, longest) - from, never below 0; to_bar = from_bar = 0 is the whole row.
int32_t tail_longest(int32_t from_bar, int32_t to_bar, int32_t longest);

// bt_set_tail_row(e, 1) with a row that does not fit, and the staging of one unit (a dataset row of P
// lanes in all-lanes mode, else a lane) above the budget.
std::string tail_row_refusal(int64_t longest_n, size_t row_bytes, size_t lds_row_bytes);
std::string tail_budget_refusal(bool all_lanes, size_t need_bytes, size_t budget);

}  // namespace bt
