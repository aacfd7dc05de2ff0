// k_replay.hip — replay of chosen (symbol, parameter) lanes: trades, position and equity curve
// (bt_replay, include/bt.h). A third device implementation of docs/oracle_spec.md §4/§5 beside
// the sweep kernels (k_sma.hip, k_tile.hip): one wave64 workgroup per requested lane, walking the
// symbol in 64-bar tiles with lane = bar.
//
// Per tile, data-parallel: coalesced loads of c (h, l for Bollinger) and of the bar that leaves
// each window (a second coalesced stream at t - w), window sums advanced by wave scans of
// c_t - c_(t-w) with ONE carried value per sum (no prefix ring, so no grid-dependent LDS: any
// window bt_engine_create accepts replays), the decision predicates as 64-bit ballots, q_t / q2_t
// through fixed_ret. Sequential: only the EMA chain (a 64-step wave-uniform loop, each lane
// keeping its own bar's value) and the state machine, a wave-uniform loop that advances once per
// EVENT (entry, exit, flip) and finds the next one with ballots restricted to the lanes after the
// cursor. Each event updates the per-lane (pos, entry_px, realized) of the lanes at and after it;
// E_t, pos_t, exposure, S1/S2, peak (prefix max) and mdd follow lane-parallel with wave
// reductions, carried across tiles.
#include "device_common.h"

namespace bt {

namespace {

__device__ __forceinline__ uint64_t from_bit(int i) { return i >= 64 ? 0ull : (i <= 0 ? ~0ull : ~0ull << i); }

__device__ __forceinline__ int32_t lane_i32(int32_t x, int i) {
    return (int32_t)__builtin_amdgcn_readlane((uint32_t)x, __builtin_amdgcn_readfirstlane(i));
}

__device__ __forceinline__ int64_t wave_sum_i64(int64_t x) { return lane63_i64(wave_iscan_i64(x)); }

// Wave64 inclusive prefix maximum of int64.
__device__ __forceinline__ int64_t wave_maxscan_i64(int64_t x, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t y = __shfl_up((long long)x, d, 64);
        if (lane >= d) x = y > x ? y : x;
    }
    return x;
}

}  // namespace

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

    // ---- the lane's parameters (param order of include/bt.h)
    int32_t w1 = 1, w2 = 1;          // SMA f, s; EMA+OLS span n, window w; Bollinger w (w1)
    int32_t sl_bps = 0, tp_bps = 0;
    int64_t kn = 0;
    if (STRAT == BT_BOLL) {
        int32_t p = L.param;
        tp_bps = g.d[p % g.nd];
        p /= g.nd;
        sl_bps = g.c[p % g.nc];
        p /= g.nc;
        kn = g.b[p % g.nb];
        w1 = g.a[p / g.nb];
    } else {
        w1 = g.a[L.param / g.nb];
        w2 = g.b[L.param % g.nb];
    }
    const int32_t warm = STRAT == BT_BOLL ? w1 - 1 : (w1 > w2 ? w1 : w2) - 1;
    const double alpha = 2.0 / ((double)w1 + 1.0);
    const double lo_mult = (double)(10000 - g.band_bps), hi_mult = (double)(10000 + g.band_bps);
    const i128 kd2 = (i128)((int64_t)g.k_den * g.k_den), kn2 = (i128)(kn * kn);

    // ---- state carried across tiles (wave-uniform)
    int32_t pos = 0, ebar = 0, ntr = 0;
    int64_t epx = 0, R = 0, peak = 0, mdd = 0, expo = 0, sl_lvl = 0, tp_lvl = 0;
    uint64_t hash = 0;
    i128 s1 = 0, s2 = 0;
    uint64_t cA = 0, cB = 0;         // window-sum carries (SMA F, L; EMA+OLS S, U; Bollinger Sc)
    i128 cSc2 = 0;                   // Bollinger sum of c^2
    double e_run = 0.0;              // EMA value after the previous tile's last bar

    for (int32_t t0 = 0; t0 < B; t0 += kTile) {
        const int32_t t = t0 + lane;
        const bool valid = t < B;
        const int32_t c = valid ? cs[t] : 0;
        const int32_t cp = (valid && t >= 1) ? cs[t - 1] : 1;
        const bool dec = valid && t >= warm && t <= B - 2;
        const uint64_t last = (B - 1 - t0) < kTile ? 1ull << (B - 1 - t0) : 0ull;

        // ---- per-bar predicates -> ballots
        uint64_t mA = 0, mB = 0, mC = 0, mD = 0;
        int32_t h = 0, l = 0;
        if (STRAT == BT_SMA_CROSS) {
            const int64_t la = (valid && t >= w1) ? cs[t - w1] : 0;
            const int64_t lb = (valid && t >= w2) ? cs[t - w2] : 0;
            int64_t da = (int64_t)c - la, db = (int64_t)c - lb;
            const uint64_t F = cA + (uint64_t)wave_iscan_i64(da);
            const uint64_t Lw = cB + (uint64_t)wave_iscan_i64(db);
            cA = (uint64_t)lane63_i64((int64_t)F);
            cB = (uint64_t)lane63_i64((int64_t)Lw);
            // F s and L f < 2^59 once both windows are full (windows <= 16,192, c < 2^31)
            const int64_t lhs = (int64_t)(F * (uint64_t)w2), rhs = (int64_t)(Lw * (uint64_t)w1);
            mA = __ballot(dec && lhs > rhs);   // target +1
            mB = __ballot(dec && lhs < rhs);   // target -1
        } else if (STRAT == BT_EMA_OLS) {
            // the chain: three roundings per bar, sequential by definition
            double my_e = 0.0;
#pragma unroll
            for (int i = 0; i < kTile; ++i) {
                const double ci = (double)(int32_t)__builtin_amdgcn_readlane((uint32_t)c, i);
                if (i == 0 && t0 == 0) e_run = ci;
                else e_run = e_run + alpha * (ci - e_run);
                my_e = lane == i ? e_run : my_e;
            }
            // OLS numerator from the window sums of c_k and k c_k (absolute k), mod 2^64:
            // N_t = 2 (U - (t - w + 1) S) - (w - 1) S, |N_t| < w^2 2^31
            const uint64_t lv = (valid && t >= w2) ? (uint64_t)cs[t - w2] : 0ull;
            const int64_t ds = (int64_t)((uint64_t)c - lv);
            const int64_t du = (int64_t)((uint64_t)t * (uint64_t)c - (uint64_t)(int64_t)(t - w2) * lv);
            const uint64_t S = cA + (uint64_t)wave_iscan_i64(ds);
            const uint64_t U = cB + (uint64_t)wave_iscan_i64(du);
            cA = (uint64_t)lane63_i64((int64_t)S);
            cB = (uint64_t)lane63_i64((int64_t)U);
            const uint64_t Trel = U - (uint64_t)(int64_t)(t - w2 + 1) * S;
            const int64_t N = (int64_t)(2 * Trel - (uint64_t)(w2 - 1) * S);
            const double cd = (double)c, lhs = cd * 10000.0;
            const bool el = lhs < my_e * lo_mult && N >= 0;
            const bool es = !el && lhs > my_e * hi_mult && N <= 0;
            mA = __ballot(dec && el);          // flat -> long
            mB = __ballot(dec && es);          // flat -> short
            mC = __ballot(dec && cd >= my_e);  // long -> flat
            mD = __ballot(dec && cd <= my_e);  // short -> flat
        } else {
            h = valid ? hs[t] : 0;
            l = valid ? ls[t] : 0;
            const int64_t lv = (valid && t >= w1) ? cs[t - w1] : 0;
            const uint64_t Sc = cA + (uint64_t)wave_iscan_i64((int64_t)c - lv);
            cA = (uint64_t)lane63_i64((int64_t)Sc);
            // c^2 < 2^62: a 64-lane sum leaves int64, so the squares go in 32-bit halves
            const uint64_t c2 = (uint64_t)c * (uint64_t)c, l2 = (uint64_t)lv * (uint64_t)lv;
            const int64_t dh = (int64_t)(c2 >> 32) - (int64_t)(l2 >> 32);
            const int64_t dl = (int64_t)(c2 & 0xFFFFFFFFull) - (int64_t)(l2 & 0xFFFFFFFFull);
            const int64_t sh = wave_iscan_i64(dh), sw = wave_iscan_i64(dl);
            const i128 Sc2 = cSc2 + (i128)sh * ((i128)1 << 32) + (i128)sw;
            cSc2 += (i128)lane63_i64(sh) * ((i128)1 << 32) + (i128)lane63_i64(sw);
            const int64_t D = (int64_t)w1 * c - (int64_t)Sc;
            const i128 Q = (i128)w1 * Sc2 - (i128)(int64_t)Sc * (i128)(int64_t)Sc;
            const bool zt = (i128)D * (i128)D * kd2 > kn2 * Q;
            mA = __ballot(dec && D < 0 && zt);  // flat -> long
            mB = __ballot(dec && D > 0 && zt);  // flat -> short
            mC = __ballot(dec && D >= 0);       // long -> flat at c
            mD = __ballot(dec && D <= 0);       // short -> flat at c
        }

        // ---- the state machine: one iteration per event
        int32_t lpos = pos, lprev = pos;   // position after / before this lane's bar
        int64_t lentry = epx, lreal = R;
        auto close_trade = [&](int i, int64_t px) {
            R += (int64_t)pos * (px - epx);
            hash += trade_mix_et((uint32_t)ebar, (uint32_t)(t0 + i), pos > 0);
            if (ntr < o.trade_cap && lane == i) {
                bt_trade tr;
                tr.entry_bar = ebar;
                tr.exit_bar = t0 + i;
                tr.side = pos;
                tr.pad = 0;
                tr.entry_px = epx;
                tr.exit_px = px;
                o.trades[r * o.trade_cap + ntr] = tr;
            }
            ++ntr;
        };
        auto set_state = [&](int i, int32_t np, int64_t px) {
            pos = np;
            ebar = t0 + i;
            epx = px;
            if (lane >= i) {
                lpos = np;
                lentry = px;
                lreal = R;
            }
            if (lane > i) lprev = np;
        };
        int cur = 0;
        if (STRAT == BT_BOLL) {
            for (;;) {
                if (pos == 0) {
                    const uint64_t m = (mA | mB) & from_bit(cur);
                    if (!m) break;
                    const int i = __builtin_ctzll(m);
                    const int64_t ce = lane_i32(c, i);
                    const bool lg = (mA >> i) & 1;
                    set_state(i, lg ? 1 : -1, ce);
                    sl_lvl = ce * (lg ? 10000 - sl_bps : 10000 + sl_bps) / 10000;
                    tp_lvl = ce * (lg ? 10000 + tp_bps : 10000 - tp_bps) / 10000;
                    cur = i + 1;
                } else {
                    // SL before TP, both only from entry + 1; then the forced / D exit at c
                    const int first = max(cur, ebar + 1 - t0);
                    const uint64_t slm = __ballot(valid && (pos > 0 ? l <= sl_lvl : h >= sl_lvl)) & from_bit(first);
                    const uint64_t tpm = __ballot(valid && (pos > 0 ? h >= tp_lvl : l <= tp_lvl)) & from_bit(first);
                    const uint64_t dx = ((pos > 0 ? mC : mD) | last) & from_bit(cur);
                    const uint64_t m = slm | tpm | dx;
                    if (!m) break;
                    const int i = __builtin_ctzll(m);
                    const int64_t px = ((slm >> i) & 1) ? sl_lvl : ((tpm >> i) & 1) ? tp_lvl : (int64_t)lane_i32(c, i);
                    close_trade(i, px);
                    set_state(i, 0, 0);
                    cur = i + 1;   // no entry at a bar that exited
                }
            }
        } else {
            for (;;) {
                uint64_t m;
                if (STRAT == BT_SMA_CROSS) m = pos > 0 ? mB : pos < 0 ? mA : (mA | mB);
                else m = pos > 0 ? mC : pos < 0 ? mD : (mA | mB);
                m &= from_bit(cur);
                if (!m) break;
                const int i = __builtin_ctzll(m);
                const int64_t px = lane_i32(c, i);
                int32_t np = ((mA >> i) & 1) ? 1 : -1;
                if (STRAT == BT_EMA_OLS && pos != 0) np = 0;
                if (pos != 0) close_trade(i, px);
                set_state(i, np, px);
                cur = i + 1;       // one transition per bar
            }
            if (last && pos != 0) {  // forced exit at B - 1
                const int i = B - 1 - t0;
                const int64_t px = lane_i32(c, i);
                close_trade(i, px);
                set_state(i, 0, 0);
            }
        }

        // ---- accounting, lane-parallel
        const int64_t E = lreal + (int64_t)lpos * ((int64_t)c - lentry);
        if (valid) {
            if (o.equity) o.equity[r * o.pitch + t] = E;
            if (o.pos) o.pos[r * o.pitch + t] = (int8_t)lpos;
        }
        const bool held = valid && t >= 1 && lprev != 0;
        int64_t q, q2;
        fixed_ret(c, cp, q, q2);
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
        s.n_trades = ntr;
        s.status = 0;
        s.pnl = R;
        s.mdd = mdd;
        s.exposure = expo;
        s.sharpe = sharpe_fx((uint64_t)s1, (int64_t)(s1 >> 64), (uint64_t)s2, (int64_t)(s2 >> 64), B, g.sqrt_ann);
        s.hash = hash;
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
