// surface.cpp — the reductions of a run on the host (docs/surface_spec.md): bt_surface_host, the
// scalar restatement of what k_surface.hip computes on the device, and bt_surface_merge, the
// combination of aggregates of disjoint symbol sets (ranks, shards). Written from the spec with
// the compiler's __int128 and shares no code with the kernels but the split of an int128 into its
// words (host_common.h), so that the two check each other.
// Plain C++: no HIP call, builds with any host compiler.
#include "surface.h"

#include <cmath>
#include <cstring>
#include <exception>

namespace bt {

std::string surface_refusal(int64_t S, int64_t P, bool have_out, bool bounded, uint64_t total_rows) {
    if (S < 0) return "S = " + std::to_string(S) + " is negative";
    if (P < 1) return "P = " + std::to_string(P) + " is below 1";
    if (!have_out) return "agg and best are both NULL";
    if (bounded && (S > kSurfaceOfMax || S * P > kSurfaceOfMax))
        return "S*P = " + std::to_string(S) + "*" + std::to_string(P) + " exceeds 2^22 records";
    if (total_rows >= kSurfaceMaxRows)
        return std::to_string(total_rows) + " rows: dataset too large for exact int64 sums";
    return "";
}

}  // namespace bt

namespace {

using bt::i128;
using bt::refuse;
using bt::wide_join;
using bt::wide_split;

// The engine's orderable Sharpe (spec §5): the double's bits, monotone as an unsigned integer.
uint64_t sharpe_key(double x) {
    uint64_t u;
    memcpy(&u, &x, sizeof u);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ULL);
}

// qs of surface_spec §1: the clamped Sharpe in 2^-32 units, rounded half to even (the default
// rounding mode; the product is exact). A NaN, which no run produces, counts as 0.
int64_t sharpe_fixed(double sh) {
    if (sh != sh) return 0;
    const double x = sh < -32768.0 ? -32768.0 : (sh > 32768.0 ? 32768.0 : sh);
    return (int64_t)std::nearbyint(x * 4294967296.0);
}

bt_param_agg empty_agg() {
    bt_param_agg a;
    memset(&a, 0, sizeof a);
    a.sym_max = a.sym_min = -1;
    return a;
}

int64_t wrap_add(int64_t a, int64_t b) { return (int64_t)((uint64_t)a + (uint64_t)b); }

// "x (symbol id) replaces the current maximum / minimum": a greater / smaller key, ties to the lower id
bool better_max(double x, int32_t id, double cur, int32_t cur_id) {
    const uint64_t k = sharpe_key(x), c = sharpe_key(cur);
    return k > c || (k == c && id < cur_id);
}
bool better_min(double x, int32_t id, double cur, int32_t cur_id) {
    const uint64_t k = sharpe_key(x), c = sharpe_key(cur);
    return k < c || (k == c && id < cur_id);
}

// a += b for aggregates of disjoint symbol sets (surface_spec §3)
void merge_into(bt_param_agg& a, const bt_param_agg& b) {
    if (b.n_sym == 0) return;
    if (a.n_sym == 0) {
        a = b;
        return;
    }
    a.n_sym += b.n_sym;
    a.n_traded += b.n_traded;
    a.n_win += b.n_win;
    a.n_pos += b.n_pos;
    a.trades = wrap_add(a.trades, b.trades);
    a.pnl = wrap_add(a.pnl, b.pnl);
    a.exposure = wrap_add(a.exposure, b.exposure);
    if (b.mdd_max > a.mdd_max) a.mdd_max = b.mdd_max;
    if (better_max(b.sharpe_max, b.sym_max, a.sharpe_max, a.sym_max)) {
        a.sharpe_max = b.sharpe_max;
        a.sym_max = b.sym_max;
    }
    if (better_min(b.sharpe_min, b.sym_min, a.sharpe_min, a.sym_min)) {
        a.sharpe_min = b.sharpe_min;
        a.sym_min = b.sym_min;
    }
    wide_split((i128)((unsigned __int128)wide_join(a.ss1_lo, a.ss1_hi) + (unsigned __int128)wide_join(b.ss1_lo, b.ss1_hi)),
               a.ss1_lo, a.ss1_hi);
    wide_split((i128)((unsigned __int128)wide_join(a.ss2_lo, a.ss2_hi) + (unsigned __int128)wide_join(b.ss2_lo, b.ss2_hi)),
               a.ss2_lo, a.ss2_hi);
}

bt_param_agg column(int32_t S, int32_t P, int32_t p, const bt_summary* sum, const int32_t* ids) {
    bt_param_agg a = empty_agg();
    i128 ss1 = 0, ss2 = 0;
    for (int32_t s = 0; s < S; ++s) {
        const bt_summary& r = sum[(size_t)s * (size_t)P + (size_t)p];
        if (r.status != 0) continue;
        const int32_t id = ids[s];
        if (a.n_sym == 0) {
            a.mdd_max = r.mdd;
            a.sharpe_max = a.sharpe_min = r.sharpe;
            a.sym_max = a.sym_min = id;
        } else {
            if (r.mdd > a.mdd_max) a.mdd_max = r.mdd;
            if (better_max(r.sharpe, id, a.sharpe_max, a.sym_max)) {
                a.sharpe_max = r.sharpe;
                a.sym_max = id;
            }
            if (better_min(r.sharpe, id, a.sharpe_min, a.sym_min)) {
                a.sharpe_min = r.sharpe;
                a.sym_min = id;
            }
        }
        a.n_sym += 1;
        a.n_traded += r.n_trades > 0;
        a.n_win += r.pnl > 0;
        a.n_pos += r.sharpe > 0;
        a.trades = wrap_add(a.trades, r.n_trades);
        a.pnl = wrap_add(a.pnl, r.pnl);
        a.exposure = wrap_add(a.exposure, r.exposure);
        const i128 q = sharpe_fixed(r.sharpe);
        ss1 += q;
        ss2 += q * q;
    }
    wide_split(ss1, a.ss1_lo, a.ss1_hi);
    wide_split(ss2, a.ss2_lo, a.ss2_hi);
    return a;
}

}  // namespace

extern "C" {

int32_t bt_surface_host(int32_t S, int32_t P, const bt_summary* sum, const int32_t* sym_ids,
                        bt_param_agg* agg, bt_topk_rec* best) {
    try {
        const std::string why = bt::surface_refusal(S, P, agg || best, false, 0);
        if (!why.empty()) return refuse("bt_surface_host", why);
        if (S > 0 && (!sum || !sym_ids)) return refuse("bt_surface_host", "sum and sym_ids are required");
        if (agg)
            for (int32_t p = 0; p < P; ++p) agg[p] = column(S, P, p, sum, sym_ids);
        if (best)
            for (int32_t s = 0; s < S; ++s) {
                const bt_summary* row = sum + (size_t)s * (size_t)P;
                int32_t bp = 0;
                for (int32_t p = 1; p < P; ++p)  // Sharpe descending, then param ascending
                    if (sharpe_key(row[p].sharpe) > sharpe_key(row[bp].sharpe)) bp = p;
                best[s] = bt_topk_rec{row[bp].sharpe, sym_ids[s], bp, row[bp].pnl};
            }
        return 0;
    } catch (const std::exception& x) {
        return refuse("bt_surface_host", std::string("exception: ") + x.what());
    }
}

int32_t bt_surface_merge(const bt_param_agg* in, int32_t world, int32_t P, bt_param_agg* out) {
    try {
        if (world < 1) return refuse("bt_surface_merge", "world = " + std::to_string(world) + " is below 1");
        if (P < 1) return refuse("bt_surface_merge", "P = " + std::to_string(P) + " is below 1");
        if (!in || !out) return refuse("bt_surface_merge", "in and out are required");
        for (int32_t p = 0; p < P; ++p) {
            bt_param_agg a = empty_agg();
            for (int32_t w = 0; w < world; ++w) merge_into(a, in[(size_t)w * (size_t)P + (size_t)p]);
            out[p] = a;
        }
        return 0;
    } catch (const std::exception& x) {
        return refuse("bt_surface_merge", std::string("exception: ") + x.what());
    }
}

}  // extern "C"
