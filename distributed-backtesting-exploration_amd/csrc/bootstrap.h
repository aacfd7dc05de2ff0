// bootstrap.h — host side of the bootstrap reality check (docs/bootstrap_spec.md): the record
// layouts, the argument rules of bt_bootstrap / bt_bootstrap_of and what bootstrap.cpp shares with
// analysis.cpp. No HIP type: bootstrap.cpp builds with a plain host compiler (tests/asan).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "host_common.h"

static_assert(sizeof(bt_boot_lane) == 48 && offsetof(bt_boot_lane, m1) == 16 && offsetof(bt_boot_lane, m2) == 32,
              "bt_boot_lane layout");
static_assert(sizeof(bt_boot_group) == 24 && offsetof(bt_boot_group, best_lane) == 8 &&
                  offsetof(bt_boot_group, n_ge) == 16,
              "bt_boot_group layout");

namespace bt {

constexpr int32_t kBootMaxT = 1 << 22;      // bars of a window, and the longest block

// What a call was given, for the rules below. `staged`: bt_bootstrap_of (no dataset, no window:
// from_bar = 0, to_bar = T).
struct BootCall {
    bool have_engine, have_dataset, staged;
    bool have_lanes;                 // list mode; a staged call: d given
    int64_t n, G;
    const int32_t* goff;             // [G + 1] or NULL
    int64_t from_bar, to_bar;        // as passed
    int64_t B, L;
    bool any_output, want_boot;
};

// Why the arguments are refused ("" = accepted), in the order the call checks them: the engine, the
// dataset, the mode and n, the groups, from_bar, B, L, the outputs. The window's T is checked by
// boot_window once the rows are known.
std::string boot_refusal(const BootCall& c);

// goff[0..G] against n lanes: goff[0] = 0, strictly increasing (no empty group), goff[G] = n.
std::string boot_groups_refusal(int64_t n, int64_t G, const int32_t* goff);

// T of the window: to_bar - from_bar, or b_max for the default window from_bar = to_bar = 0.
// Refuses T < 1 and T > 2^22.
std::string boot_window(int64_t from_bar, int64_t to_bar, int64_t b_max, int32_t& T);

// The old name of increments_domain_refusal (host_common.h), kept like internal.h's ReplayLane:
// tests/asan/boot_driver.cpp builds with it.
inline std::string boot_domain_refusal(int64_t n, int64_t T, const int32_t* d) {
    return increments_domain_refusal(n, T, d);
}

// The smallest staging the call can run in against the budget.
std::string boot_budget_refusal(size_t need_bytes, size_t budget);

// A row of T + 1 words against the LDS row limit (bt_set_boot_row mode 1).
std::string boot_row_refusal(int64_t T, size_t row_bytes, size_t limit_bytes);

// Draw k (0-based) of the generator of docs/oracle_spec.md §1 with b in the place of sym.
inline uint64_t boot_draw(uint64_t seed, uint64_t b, uint64_t k) {
    const uint64_t s0 = seed ^ (b * 0x9E3779B97F4A7C15ULL);
    uint64_t z = s0 + (k + 1) * 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

}  // namespace bt
