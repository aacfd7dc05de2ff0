// k_replay.hip — replay of chosen (symbol, parameter) lanes: trades, position and equity curve
// (bt_replay, include/bt.h): one wave64 workgroup per requested lane, a LaneWalk (walk_tile.h).
// Per tile and lane-parallel, with wave reductions carried across tiles: E_t, pos_t, exposure and
// S1/S2 (tile_returns), peak and mdd over the valid bars from peak = 0 (PeakDrawdown), and the
// trade records from the walk's callback.
#include "walk_tile.h"

namespace bt {

// STRAT: bt_strategy. Block = one wave; blockIdx.x = index of the lane in this chunk.
template <int STRAT>
__global__ __launch_bounds__(64) void replay_kernel(const LaneRef* __restrict__ lanes,
                                                    const int32_t* __restrict__ high,
                                                    const int32_t* __restrict__ low,
                                                    const int32_t* __restrict__ close, const Grid g,
                                                    const ReplayOut o) {
    const int lane = (int)threadIdx.x;
    const int64_t r = (int64_t)blockIdx.x;
    const LaneRef L = lanes[r];
    LaneWalk<STRAT> lw(g, L.off, L.bars, L.param, high, low, close, lane);

    // ---- sums carried across tiles (wave-uniform)
    PeakDrawdown pd;
    int64_t expo = 0;
    i128 s1 = 0, s2 = 0;

    for (int32_t t0 = 0; t0 < L.bars; t0 += kTile) {
        const int32_t t = t0 + lane;
        const LaneTile w = lw.step(t0, [&](int i, int32_t n, int32_t ebar, int32_t side, int64_t epx, int64_t px) {
            if (n < o.trade_cap && lane == i) o.trades[r * o.trade_cap + n] = bt_trade{ebar, t0 + i, side, 0, epx, px};
        });
        if (w.valid) {
            if (o.equity) o.equity[r * o.pitch + t] = w.E;
            if (o.pos) o.pos[r * o.pitch + t] = (int8_t)w.lpos;
        }
        const TileReturns ret = tile_returns(w, t);
        s1 += (i128)wave_sum_i64(ret.r1);
        s2 += (i128)wave_sum_i64(ret.r2);
        expo += __popcll(ret.held);
        pd.add(w.E, w.valid, lane);
    }

    if (lane == 0) {
        bt_summary s;
        s.n_trades = lw.st.ntr;
        s.status = 0;
        s.pnl = lw.st.R;
        s.mdd = pd.mdd;
        s.exposure = expo;
        s.sharpe = sharpe_fx(s1, s2, L.bars, g.sqrt_ann);
        s.hash = lw.st.hash;
        o.sum[r] = s;
    }
}

hipError_t launch_replay(const LaneRef* lanes, int32_t n, const int32_t* high, const int32_t* low,
                         const int32_t* close, const Grid& g, const ReplayOut& o, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    launch_by_strategy(g.strategy, [&](auto strat) {
        hipLaunchKernelGGL(replay_kernel<decltype(strat)::value>, dim3((unsigned)n), dim3(kTile), 0, st, lanes, high,
                           low, close, g, o);
    });
    return hipGetLastError();
}

}  // namespace bt
