// k_replay.hip — replay of chosen (symbol, parameter) lanes: trades, position and equity curve
// (bt_replay, include/bt.h): one wave64 workgroup per requested lane, walking the symbol in 64-bar
// tiles with lane = bar. The tile walk (loads, window scans, ballots, the event loop and the
// per-lane (pos, entry_px, realized)) is walk_tile.h, shared with k_walkfwd.hip; here follow, per
// tile and lane-parallel with wave reductions carried across tiles, E_t, pos_t, exposure, S1/S2
// (q_t / q2_t through fixed_ret), peak (prefix max) and mdd, and the trade records.
#include "walk_tile.h"

namespace bt {

// STRAT: bt_strategy. Block = one wave; blockIdx.x = index of the lane in this chunk.
template <int STRAT>
__global__ __launch_bounds__(64) void replay_kernel(const ReplayLane* __restrict__ lanes,
                                                    const int32_t* __restrict__ high,
                                                    const int32_t* __restrict__ low,
                                                    const int32_t* __restrict__ close, const Grid g,
                                                    const ReplayOut o) {
    const int lane = (int)threadIdx.x;
    const int64_t r = (int64_t)blockIdx.x;
    const ReplayLane L = lanes[r];
    const int32_t B = L.bars;
    const int32_t* __restrict__ cs = close + L.off;
    const int32_t* __restrict__ hs = STRAT == BT_BOLL ? high + L.off : nullptr;
    const int32_t* __restrict__ ls = STRAT == BT_BOLL ? low + L.off : nullptr;
    const LaneParams<STRAT> P(g, L.param);

    // ---- state carried across tiles (wave-uniform)
    WalkState st;
    int64_t peak = 0, mdd = 0, expo = 0;
    i128 s1 = 0, s2 = 0;

    for (int32_t t0 = 0; t0 < B; t0 += kTile) {
        const int32_t t = t0 + lane;
        TileLanes w;
        walk_tile<STRAT>(P, g, st, cs, hs, ls, B, t0, lane, w, [&](int i, int32_t n, int32_t ebar, int32_t side, int64_t epx, int64_t px) {
            if (n < o.trade_cap && lane == i) {
                bt_trade tr;
                tr.entry_bar = ebar;
                tr.exit_bar = t0 + i;
                tr.side = side;
                tr.pad = 0;
                tr.entry_px = epx;
                tr.exit_px = px;
                o.trades[r * o.trade_cap + n] = tr;
            }
        });
        const bool valid = w.valid;
        const int32_t c = w.c, lpos = w.lpos, lprev = w.lprev;

        // ---- accounting, lane-parallel
        const int64_t E = w.lreal + (int64_t)lpos * ((int64_t)c - w.lentry);
        if (valid) {
            if (o.equity) o.equity[r * o.pitch + t] = E;
            if (o.pos) o.pos[r * o.pitch + t] = (int8_t)lpos;
        }
        const bool held = valid && t >= 1 && lprev != 0;
        int64_t q, q2;
        fixed_ret(c, w.cp, q, q2);
        // |q|, q2 <= 2^56 (spec §3): a tile's partial sums fit int64
        s1 += (i128)wave_sum_i64(held ? (int64_t)lprev * q : 0);
        s2 += (i128)wave_sum_i64(held ? q2 : 0);
        expo += __popcll(__ballot(held));
        const int64_t pm = wave_maxscan_i64(valid ? E : INT64_MIN, lane);
        const int64_t pk = pm > peak ? pm : peak;
        const int64_t dd = wave_maxscan_i64(valid ? pk - E : 0, lane);
        const int64_t tile_dd = lane63_i64(dd);
        mdd = tile_dd > mdd ? tile_dd : mdd;
        peak = lane63_i64(pk);
    }

    if (lane == 0) {
        bt_summary s;
        s.n_trades = st.ntr;
        s.status = 0;
        s.pnl = st.R;
        s.mdd = mdd;
        s.exposure = expo;
        s.sharpe = sharpe_fx((uint64_t)s1, (int64_t)(s1 >> 64), (uint64_t)s2, (int64_t)(s2 >> 64), B, g.sqrt_ann);
        s.hash = st.hash;
        o.sum[r] = s;
    }
}

hipError_t launch_replay(const ReplayLane* lanes, int32_t n, const int32_t* high, const int32_t* low,
                         const int32_t* close, const Grid& g, const ReplayOut& o, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const dim3 grid((unsigned)n), block(kTile);
    switch (g.strategy) {
        case BT_SMA_CROSS:
            hipLaunchKernelGGL(replay_kernel<BT_SMA_CROSS>, grid, block, 0, st, lanes, high, low, close, g, o);
            break;
        case BT_EMA_OLS:
            hipLaunchKernelGGL(replay_kernel<BT_EMA_OLS>, grid, block, 0, st, lanes, high, low, close, g, o);
            break;
        default:
            hipLaunchKernelGGL(replay_kernel<BT_BOLL>, grid, block, 0, st, lanes, high, low, close, g, o);
            break;
    }
    return hipGetLastError();
}

}  // namespace bt
