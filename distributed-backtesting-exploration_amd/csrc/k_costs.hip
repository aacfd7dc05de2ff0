// k_costs.hip — net of costs on the device: every lane under a ladder of fee levels (bt_costs,
// include/bt.h; semantics: docs/costs_spec.md).
//
// cost_walk_kernel: one wave64 workgroup per lane, a LaneWalk (walk_tile.h) over its whole series,
// lane = bar. The walk's on_trade callback notes each closing trade (entry price, exit price, gross
// pnl) in the lane of its exit bar, as k_tstats.hip does. Per tile the level-independent work is
// done once: the exit flag (the walk's exit ballot) and the entry flag (a valid lane whose position
// is not flat and differs from the one before the bar; every entry fills at the bar's close), the
// two fill prices and the turnover. Then a wave-uniform loop runs over the C levels with (fixed,
// bps) as scalars from the level table, which travels by value in the kernel arguments: the bar's
// fee, its inclusive scan on top of the carried fee total, N = E - F, the prefix maximum on top of
// the carried net peak, the drawdown (its first bar on strict improvement only), the ballot of the
// bars under water, the squares of the net increments summed in 32-bit halves into the carried
// int128, and the net trade figures from ballots and wave sums over the exit lanes. Level j's
// carried state (eighteen words) lives in lane j of a few VGPRs: read with a readlane at the
// uniform j, written back under lane == j. Lane 0 writes every record field by field. No LDS, no
// scratch.
//
// cost_agg_kernel: threads along q = p * C + j, grid y over slices of a chunk's rows; each thread
// adds its slice's records of (parameter, level) q in registers and then into agg[q] with integer
// atomic adds and one atomic maximum of non-negative values, so any order of slices and chunks
// leaves the same bits.
#include "plan.h"
#include "walk_tile.h"

namespace bt {

namespace {

// floor(px * bps / 10000) for px < 2^32, bps <= 1000. x = px * bps < 2^42 is exact in a double and
// so is x + 0.5; (x + 0.5) / 10000 lies at least 0.5 / 10000 = 2^-14.3 away from every integer, and
// the product with the rounded 1e-4 errs by less than 2^-52 * 2^29 = 2^-23: the truncation is the
// floor. No 64-bit division.
__device__ __forceinline__ uint32_t bps_part(uint32_t px, uint32_t bps) {
    const uint64_t x = (uint64_t)px * bps;
    return (uint32_t)(((double)x + 0.5) * 1e-4);
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
__global__ __launch_bounds__(64) void cost_walk_kernel(const CostArgs a, const CostLevels lv,
                                                       const int32_t* __restrict__ high,
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
    const int32_t B = L.bars, C = a.C;
    LaneWalk<STRAT> lw(g, L.off, L.bars, L.param, high, low, close, lane);

    // ---- carried across tiles, level j's in lane j: the fee total, the net peak and drawdown ...
    int64_t vF = 0, vPeak = 0, vMdd = 0;
    int32_t vMddBar = -1, vUw = 0;
    // ... the int128 sum of squared net increments, and the net trade figures
    uint64_t vS2lo = 0;
    int64_t vS2hi = 0, vWin = 0, vLoss = 0;
    int32_t vNwin = 0, vNloss = 0;
    int64_t turnover = 0;            // wave-uniform: the same on every level

    for (int32_t t0 = 0; t0 < B; t0 += kTile) {
        // per lane: the trade that closed at the lane's bar (a bar closes at most one trade)
        uint32_t t_epx = 0, t_xpx = 0;
        int32_t t_pnl = 0;
        const LaneTile w = lw.step(t0, [&](int i, int32_t, int32_t, int32_t side, int64_t epx, int64_t px) {
            if (lane == i) {
                t_pnl = (int32_t)(side > 0 ? px - epx : epx - px);   // |pnl| < 2^31
                t_epx = (uint32_t)epx;                               // fill prices < 2^32
                t_xpx = (uint32_t)px;
            }
        });
        // ---- once per tile: the fills of the lane's bar
        const bool in = w.valid;
        const bool ex = (w.exits >> lane) & 1;
        const bool en = in && w.lpos != 0 && w.lpos != w.lprev;
        const uint64_t entries = __ballot(en);
        const uint32_t pe = en ? (uint32_t)w.c : 0u, px = ex ? t_xpx : 0u;
        if (entries | w.exits) turnover += wave_sum_i64((int64_t)pe + (int64_t)px);

        // ---- per level
        for (int j = 0; j < C; ++j) {
            const uint32_t fixed = (uint32_t)lv.fixed[j], bps = (uint32_t)lv.bps[j];
            // the bar's fee: below 2^30 with two fills
            uint32_t f_en = 0, f_ex = 0;
            if (entries) f_en = en ? fixed + bps_part(pe, bps) : 0u;
            if (w.exits) f_ex = ex ? fixed + bps_part(px, bps) : 0u;
            const uint32_t f = f_en + f_ex;
            int64_t F = lane_i64(vF, j);
            if (entries | w.exits) F += wave_iscan_i64((int64_t)f);
            const int64_t N = w.E - F;

            // every lane's net peak_t and drawdown; lanes with t >= B hold the peak before them and 0
            const int64_t peak = lane_i64(vPeak, j);
            const int64_t pm = wave_maxscan_i64(in ? N : INT64_MIN, lane);
            const int64_t pk = pm > peak ? pm : peak;
            const int64_t dd = in ? pk - N : 0;
            const int64_t ddmax = lane63_i64(wave_maxscan_i64(dd, lane));
            int64_t mdd = lane_i64(vMdd, j);
            int32_t mdd_bar = lane_i32(vMddBar, j);
            if (ddmax > mdd) {          // strictly: of equal drawdowns the first bar stays
                mdd = ddmax;
                mdd_bar = t0 + __builtin_ctzll(__ballot(dd == ddmax));
            }
            const int32_t uw = lane_i32(vUw, j) + __popcll(__ballot(dd > 0));

            // (N_t - N_(t-1))^2 < 2^64, and a tile's sum of them leaves int64: in 32-bit halves
            const int64_t nn = in ? w.d - (int64_t)f : 0;
            const uint32_t an = (uint32_t)(nn < 0 ? -nn : nn);   // |n_t| < 2^32
            const uint64_t n2 = (uint64_t)an * (uint64_t)an;
            const int64_t sh = wave_sum_i64((int64_t)(n2 >> 32)), sl = wave_sum_i64((int64_t)(n2 & 0xFFFFFFFFull));
            const i128 s2 = wide_join(lane_i64((int64_t)vS2lo, j), lane_i64(vS2hi, j)) + (i128)sh * ((i128)1 << 32) + (i128)sl;

            // the trades that closed in the tile, net of both fills
            int32_t n_win = lane_i32(vNwin, j), n_loss = lane_i32(vNloss, j);
            int64_t win = lane_i64(vWin, j), loss = lane_i64(vLoss, j);
            if (w.exits) {
                const uint32_t f_open = fixed + bps_part(t_epx, bps);
                const int64_t net = ex ? (int64_t)t_pnl - (int64_t)f_open - (int64_t)f_ex : 0;
                const uint64_t wins = __ballot(net > 0), losses = __ballot(net < 0);
                n_win += __popcll(wins);
                n_loss += __popcll(losses);
                if (wins) win += wave_sum_i64(net > 0 ? net : 0);
                if (losses) loss += wave_sum_i64(net < 0 ? -net : 0);
            }

            const int64_t F_end = lane63_i64(F), pk_end = lane63_i64(pk);
            if (lane == j) {
                vF = F_end;
                vPeak = pk_end;
                vMdd = mdd;
                vMddBar = mdd_bar;
                vUw = uw;
                vS2lo = wide_lo(s2);
                vS2hi = wide_hi(s2);
                vNwin = n_win;
                vNloss = n_loss;
                vWin = win;
                vLoss = loss;
            }
        }
    }

    for (int j = 0; j < C; ++j) {
        const int64_t fees = lane_i64(vF, j), mdd = lane_i64(vMdd, j), win = lane_i64(vWin, j), loss = lane_i64(vLoss, j);
        const int64_t s2lo = lane_i64((int64_t)vS2lo, j), s2hi = lane_i64(vS2hi, j);
        const int32_t mdd_bar = lane_i32(vMddBar, j), uw = lane_i32(vUw, j);
        const int32_t n_win = lane_i32(vNwin, j), n_loss = lane_i32(vNloss, j);
        if (lane == 0) {            // field by field into global memory: no private copy of the record
            bt_cost_rec* __restrict__ o = a.rec + (int64_t)blockIdx.x * C + j;
            o->n_trades = lw.st.ntr;
            o->n_win = n_win;
            o->n_loss = n_loss;
            o->n_bars = B;
            o->mdd_bar = mdd_bar;
            o->underwater_bars = uw;
            o->pnl = lw.st.R - fees;   // every position is closed by B - 1: E_(B-1) is the realized pnl
            o->fees = fees;
            o->turnover = turnover;
            o->mdd = mdd;
            o->win_sum = win;
            o->loss_sum = loss;
            o->s2_lo = (uint64_t)s2lo;
            o->s2_hi = s2hi;
        }
    }
}

constexpr int kCostAggWaves = 4;     // the reduction block is at most this many waves

__global__ __launch_bounds__(kCostAggWaves * 64) void cost_agg_kernel(const CostArgs a, const int32_t slices) {
    const int64_t PC = (int64_t)a.P * a.C;
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t per = (a.n_rows + slices - 1) / slices;
    const int32_t r0 = (int32_t)blockIdx.y * per, r1 = min(r0 + per, a.n_rows);
    if (q >= PC || r0 >= r1) return;
    int32_t n_traded = 0, n_profit = 0;
    int64_t trades = 0, pnl = 0, fees = 0, mdd_max = 0;
    for (int32_t r = r0; r < r1; ++r) {
        const bt_cost_rec& x = a.rec[(int64_t)r * PC + q];
        n_traded += x.n_trades > 0 ? 1 : 0;
        n_profit += x.pnl > 0 ? 1 : 0;
        trades += x.n_trades;
        pnl += x.pnl;
        fees += x.fees;
        mdd_max = x.mdd > mdd_max ? x.mdd : mdd_max;
    }
    bt_cost_agg* __restrict__ o = a.agg + q;
    atomicAdd(&o->n_sym, r1 - r0);
    atomicAdd(&o->n_traded, n_traded);
    atomicAdd(&o->n_profit, n_profit);
    atomic_add_i64(&o->trades, trades);
    atomic_add_i64(&o->pnl, pnl);
    atomic_add_i64(&o->fees, fees);
    atomic_max_i64(&o->mdd_max, mdd_max);
}

hipError_t launch_cost_walk(const CostArgs& a, const CostLevels& lv, const int32_t* high, const int32_t* low,
                            const int32_t* close, const Grid& g, hipStream_t st) {
    const int64_t n = a.lanes ? (int64_t)a.n : (int64_t)a.n_rows * a.P;
    if (n <= 0) return hipSuccess;
    launch_by_strategy(g.strategy, [&](auto strat) {
        hipLaunchKernelGGL(cost_walk_kernel<decltype(strat)::value>, dim3((unsigned)n), dim3(kTile), 0, st, a, lv, high,
                           low, close, g);
    });
    return hipGetLastError();
}

hipError_t launch_cost_agg(const CostArgs& a, const CostsPlan& pl, hipStream_t st) {
    static_assert(kCostAggWaves * 64 >= 256, "plan_costs: agg_block is at most 256");
    if (a.n_rows <= 0) return hipSuccess;
    const dim3 grid((unsigned)pl.agg_pblocks, (unsigned)pl.agg_slices), block((unsigned)pl.agg_block);
    hipLaunchKernelGGL(cost_agg_kernel, grid, block, 0, st, a, pl.agg_slices);
    return hipGetLastError();
}

}  // namespace bt
