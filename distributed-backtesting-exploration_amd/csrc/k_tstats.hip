// k_tstats.hip — per-lane trade statistics and drawdown timing on the device (bt_trade_stats,
// include/bt.h; semantics: docs/tradestats_spec.md).
//
// tstats_walk_kernel: one wave64 workgroup per lane, a LaneWalk (walk_tile.h) over its whole
// series. The walk's on_trade callback notes each closing trade in the lane of its exit bar; after
// the tile a wave-uniform loop over the exit ballot reads them back and updates the trade figures,
// scalars carried across tiles: counts, sums, extremes, the int128 sum of squares and the two
// streak counters (inside the walk's event loop the same accounting measured 3 % slower on the
// Bollinger shard). The drawdown figures come per tile from LaneTile::E: the prefix maximum on top of the
// carried peak (as PeakDrawdown takes it) gives every lane its peak_t; a lane whose peak_t exceeds
// that of the lane below it (lane 0: the carry) is a strict new peak; the tile's largest drawdown
// replaces the carried one only when strictly larger, at its first lane, and its peak bar is the
// last strict new peak at or before that lane, else the carried one; the ballot of the lanes with
// E_t < peak_t gives the bars under water and, with a carried run length, their longest run. Lane 0
// writes the record once, field by field. No LDS, no scratch.
//
// tstats_agg_kernel: threads along p, grid y over slices of a chunk's rows; each thread adds its
// slice's records of parameter p in registers and then into agg[p] with integer atomic adds and
// maxima (the int128 sum as an add of the low word whose wrap carries into the high word), so any
// order of slices and chunks leaves the same bits.
#include "plan.h"
#include "walk_tile.h"

namespace bt {

namespace {

// The longest run of set bits in x, for x != ~0 (a run of at most 63). y_k has bit i set iff bits
// i - k + 1 .. i are all set: y_(a+b) = y_a & (y_b << a). p[j] = y_(2^j) by doubling, then the
// length is built from its highest bit down.
__device__ __forceinline__ int longest_run(uint64_t x) {
    uint64_t p[6];
    p[0] = x;
#pragma unroll
    for (int j = 0; j < 5; ++j) p[j + 1] = p[j] & (p[j] << (1 << j));
    int len = 0;
    uint64_t cur = ~0ull;   // y_0
#pragma unroll
    for (int j = 5; j >= 0; --j) {
        const uint64_t cand = cur & (p[j] << len);
        if (cand) cur = cand, len += 1 << j;
    }
    return len;
}

__device__ __forceinline__ void atomic_add_i64(int64_t* p, int64_t v) {
    atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}
// of values that are never negative
__device__ __forceinline__ void atomic_max_i64(int64_t* p, int64_t v) {
    atomicMax(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}

}  // namespace

// STRAT: bt_strategy. Block = one wave; blockIdx.x = the request's index (list mode) or
// row * P + param of the chunk (all-lanes mode).
template <int STRAT>
__global__ __launch_bounds__(64) void tstats_walk_kernel(const TsArgs a, const int32_t* __restrict__ high,
                                                         const int32_t* __restrict__ low,
                                                         const int32_t* __restrict__ close, const Grid g) {
    const int lane = (int)threadIdx.x;
    LaneRef L;
    if (a.lanes) {
        L = a.lanes[blockIdx.x];
    } else {
        const SymDesc sd = a.syms[blockIdx.x / (uint32_t)a.P];
        L = LaneRef{sd.off, sd.bars, (int32_t)(blockIdx.x % (uint32_t)a.P)};
    }
    const int32_t B = L.bars;
    LaneWalk<STRAT> lw(g, L.off, L.bars, L.param, high, low, close, lane);

    // ---- carried across tiles (wave-uniform): the trade figures ...
    int32_t n_win = 0, n_loss = 0, n_long = 0, n_long_win = 0;
    int32_t win_run = 0, loss_run = 0, max_win_streak = 0, max_loss_streak = 0;
    int32_t hold_sum = 0, hold_win = 0, hold_max = 0;
    int64_t gross_win = 0, gross_loss = 0;
    int32_t max_win = 0, max_loss = 0;
    int32_t t_pnl = 0, t_hold = 0;   // per lane: the trade that closed at the lane's bar
    i128 sq = 0;
    // ... and the drawdown: peak_at is the first bar that holds the running peak (E_0 = 0)
    int64_t peak = 0, mdd = 0;
    int32_t mdd_bar = -1, peak_bar = -1, peak_at = 0;
    int32_t uw_bars = 0, uw_max = 0, uw_run = 0;

    for (int32_t t0 = 0; t0 < B; t0 += kTile) {
        // the walk's callback only notes the trade in the lane of its exit bar (a bar closes at
        // most one trade); the accounting below reads it back, outside the walk's event loop
        const LaneTile w = lw.step(t0, [&](int i, int32_t, int32_t ebar, int32_t side, int64_t epx, int64_t px) {
            if (lane == i) {
                t_pnl = (int32_t)(side > 0 ? px - epx : epx - px);   // |pnl| < 2^31
                t_hold = ((t0 + i - ebar) << 1) | (side > 0 ? 1 : 0);
            }
        });
        for (uint64_t m = w.exits; m; m &= m - 1) {
            const int i = __builtin_ctzll(m);
            const int32_t pnl = lane_i32(t_pnl, i), hs = lane_i32(t_hold, i);
            const int32_t hold = hs >> 1, lg = hs & 1;
            hold_sum += hold;
            hold_max = hold > hold_max ? hold : hold_max;
            n_long += lg;
            sq += (i128)((int64_t)pnl * pnl);
            if (pnl > 0) {
                n_win += 1;
                n_long_win += lg;
                hold_win += hold;
                gross_win += pnl;
                max_win = pnl > max_win ? pnl : max_win;
                loss_run = 0;
                win_run += 1;
                max_win_streak = win_run > max_win_streak ? win_run : max_win_streak;
            } else if (pnl < 0) {
                n_loss += 1;
                gross_loss -= pnl;
                max_loss = -pnl > max_loss ? -pnl : max_loss;
                win_run = 0;
                loss_run += 1;
                max_loss_streak = loss_run > max_loss_streak ? loss_run : max_loss_streak;
            } else {                // a flat trade ends both runs
                win_run = loss_run = 0;
            }
        }

        // every lane's peak_t and drawdown; lanes with t >= B hold the peak before them and 0
        const bool in = w.valid;
        const int64_t pm = wave_maxscan_i64(in ? w.E : INT64_MIN, lane);
        const int64_t pk = pm > peak ? pm : peak;
        const int64_t below = lane_below_i64(pk, lane);   // by every lane
        const uint64_t newpk = __ballot(pk > (lane == 0 ? peak : below));
        const int64_t dd = in ? pk - w.E : 0;
        const int64_t ddmax = lane63_i64(wave_maxscan_i64(dd, lane));
        if (ddmax > mdd) {          // strictly: of equal drawdowns the first bar stays
            mdd = ddmax;
            const int j = __builtin_ctzll(__ballot(dd == ddmax));
            mdd_bar = t0 + j;
            const uint64_t m = newpk & ~from_bit(j + 1);
            peak_bar = m ? t0 + 63 - __builtin_clzll(m) : peak_at;
        }
        if (newpk) peak_at = t0 + 63 - __builtin_clzll(newpk);
        peak = lane63_i64(pk);

        // bars under water, and their longest run with the run that reaches into this tile
        const uint64_t uw = __ballot(dd > 0);
        uw_bars += __popcll(uw);
        if (uw == ~0ull) {          // wholly under water: the run goes on
            uw_run += kTile;
            uw_max = uw_run > uw_max ? uw_run : uw_max;
        } else {
            const int first = uw_run + __builtin_ctzll(~uw), inner = longest_run(uw);
            const int most = first > inner ? first : inner;
            uw_max = most > uw_max ? most : uw_max;
            uw_run = __builtin_clzll(~uw);
        }
    }

    if (lane == 0) {                // field by field into global memory: no private copy of the record
        bt_tstats* __restrict__ o = a.rec + blockIdx.x;
        o->n_trades = lw.st.ntr;
        o->n_win = n_win;
        o->n_loss = n_loss;
        o->status = 0;
        o->n_long = n_long;
        o->n_long_win = n_long_win;
        o->max_win_streak = max_win_streak;
        o->max_loss_streak = max_loss_streak;
        o->hold_sum = hold_sum;
        o->hold_win = hold_win;
        o->hold_max = hold_max;
        o->n_bars = B;
        o->gross_win = gross_win;
        o->gross_loss = gross_loss;
        o->max_win = max_win;
        o->max_loss = max_loss;
        wide_split(sq, o->sq_lo, o->sq_hi);
        o->mdd = mdd;
        o->mdd_bar = mdd_bar;
        o->peak_bar = peak_bar;
        o->underwater_bars = uw_bars;
        o->max_underwater = uw_max;
        o->hash = lw.st.hash;
    }
}

constexpr int kAggWaves = 4;         // the reduction block is at most this many waves

__global__ __launch_bounds__(kAggWaves * 64) void tstats_agg_kernel(const TsArgs a, const int32_t slices) {
    const int32_t p = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    const int32_t per = (a.n_rows + slices - 1) / slices;
    const int32_t r0 = (int32_t)blockIdx.y * per, r1 = min(r0 + per, a.n_rows);
    if (p >= a.P || r0 >= r1) return;
    int32_t n_traded = 0, max_win_streak = 0, max_loss_streak = 0, hold_max = 0, max_underwater = 0;
    int64_t n_trades = 0, n_win = 0, n_loss = 0, n_long = 0, n_long_win = 0, hold_sum = 0, hold_win = 0;
    int64_t gross_win = 0, gross_loss = 0, max_win = 0, max_loss = 0, mdd_max = 0;
    i128 sq = 0;
    for (int32_t r = r0; r < r1; ++r) {
        const bt_tstats& x = a.rec[(int64_t)r * a.P + p];
        n_traded += x.n_trades > 0 ? 1 : 0;
        max_win_streak = max(max_win_streak, x.max_win_streak);
        max_loss_streak = max(max_loss_streak, x.max_loss_streak);
        hold_max = max(hold_max, x.hold_max);
        max_underwater = max(max_underwater, x.max_underwater);
        n_trades += x.n_trades;
        n_win += x.n_win;
        n_loss += x.n_loss;
        n_long += x.n_long;
        n_long_win += x.n_long_win;
        hold_sum += x.hold_sum;
        hold_win += x.hold_win;
        gross_win += x.gross_win;
        gross_loss += x.gross_loss;
        max_win = x.max_win > max_win ? x.max_win : max_win;
        max_loss = x.max_loss > max_loss ? x.max_loss : max_loss;
        mdd_max = x.mdd > mdd_max ? x.mdd : mdd_max;
        sq += wide_join(x.sq_lo, x.sq_hi);
    }
    bt_tstats_agg* __restrict__ o = a.agg + p;
    atomicAdd(&o->n_sym, r1 - r0);
    atomicAdd(&o->n_traded, n_traded);
    atomicMax(&o->max_win_streak, max_win_streak);
    atomicMax(&o->max_loss_streak, max_loss_streak);
    atomicMax(&o->hold_max, hold_max);
    atomicMax(&o->max_underwater, max_underwater);
    atomic_add_i64(&o->n_trades, n_trades);
    atomic_add_i64(&o->n_win, n_win);
    atomic_add_i64(&o->n_loss, n_loss);
    atomic_add_i64(&o->n_long, n_long);
    atomic_add_i64(&o->n_long_win, n_long_win);
    atomic_add_i64(&o->hold_sum, hold_sum);
    atomic_add_i64(&o->hold_win, hold_win);
    atomic_add_i64(&o->gross_win, gross_win);
    atomic_add_i64(&o->gross_loss, gross_loss);
    atomic_max_i64(&o->max_win, max_win);
    atomic_max_i64(&o->max_loss, max_loss);
    atomic_max_i64(&o->mdd_max, mdd_max);
    // the int128 sum: the low word's wrap carries into the high word; whatever the order of the
    // adds, the carries number floor(sum of the low words / 2^64)
    const unsigned long long lo = wide_lo(sq);
    const unsigned long long old = atomicAdd(reinterpret_cast<unsigned long long*>(&o->sq_lo), lo);
    atomic_add_i64(&o->sq_hi, wide_hi(sq) + (old + lo < old ? 1 : 0));
}

hipError_t launch_tstats_walk(const TsArgs& a, const int32_t* high, const int32_t* low, const int32_t* close,
                              const Grid& g, hipStream_t st) {
    const int64_t n = a.lanes ? (int64_t)a.n : (int64_t)a.n_rows * a.P;
    if (n <= 0) return hipSuccess;
    launch_by_strategy(g.strategy, [&](auto strat) {
        hipLaunchKernelGGL(tstats_walk_kernel<decltype(strat)::value>, dim3((unsigned)n), dim3(kTile), 0, st, a, high,
                           low, close, g);
    });
    return hipGetLastError();
}

hipError_t launch_tstats_agg(const TsArgs& a, const TstatsPlan& pl, hipStream_t st) {
    static_assert(kAggWaves * 64 >= 256, "plan_tstats: agg_block is at most 256");
    if (a.n_rows <= 0) return hipSuccess;
    const dim3 grid((unsigned)pl.agg_pblocks, (unsigned)pl.agg_slices), block((unsigned)pl.agg_block);
    hipLaunchKernelGGL(tstats_agg_kernel, grid, block, 0, st, a, pl.agg_slices);
    return hipGetLastError();
}

}  // namespace bt
