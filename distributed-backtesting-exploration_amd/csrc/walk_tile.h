// walk_tile.h — what the lane kernels share (k_replay.hip replay_kernel, k_walkfwd.hip
// wf_walk_kernel, k_portfolio.hip pf_walk_kernel, k_gram.hip gram_walk_kernel): one (symbol,
// parameter) lane walked by one wave64 workgroup in 64-bar tiles, lane = bar. A device
// implementation of docs/oracle_spec.md §4/§5 beside the sweep kernels (k_sma.hip, k_ema.hip,
// k_boll.hip).
//
// A lane kernel constructs a LaneWalk<STRAT> from its LaneRef and loops over step(t0) from tile 0
// (the state needs every bar before those it accounts); step() walks the tile (walk_tile) and
// gives every lane its bar's position, equity E_t and increment d_t = E_t - E_(t-1). The replay
// and the walk-forward folds account a tile with tile_returns and a PeakDrawdown under a lane
// mask, the portfolio and the Gram walk take d_t. launch_by_strategy picks the instantiation.
//
// Per tile, data-parallel: coalesced loads of c (h, l for Bollinger) and of the bar that leaves
// each window (a second coalesced stream at t - w), window sums advanced by wave scans of
// c_t - c_(t-w) with ONE carried value per sum (no prefix ring, so no grid-dependent LDS: any
// window bt_engine_create accepts walks), the decision predicates as 64-bit ballots. Sequential:
// only the EMA chain (a 64-step wave-uniform loop, each lane keeping its own bar's value) and the
// state machine, a wave-uniform loop that advances once per EVENT (entry, exit, flip) and finds
// the next one with ballots restricted to the lanes after the cursor. Each event updates the
// per-lane (pos, entry_px, realized) of the lanes at and after it.
#pragma once
#include "device_common.h"

namespace bt {

__device__ __forceinline__ uint64_t from_bit(int i) { return i >= 64 ? 0ull : (i <= 0 ? ~0ull : ~0ull << i); }

__device__ __forceinline__ int32_t lane_i32(int32_t x, int i) {
    return (int32_t)__builtin_amdgcn_readlane((uint32_t)x, __builtin_amdgcn_readfirstlane(i));
}

__device__ __forceinline__ int64_t lane_i64(int64_t x, int i) {
    const int j = __builtin_amdgcn_readfirstlane(i);
    const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)x, j);
    const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)((uint64_t)x >> 32), j);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// x of the lane below (lane 0: of lane 63). Not __shfl_up(x, 1), whose index is that of the first
// step of wave_maxscan_i64: sharing it, wf_walk_kernel, which never reads LaneTile::d, kept the
// six scan indices live across the tile loop (+4 VGPRs).
__device__ __forceinline__ int64_t lane_below_i64(int64_t x, int lane) {
    const int src = (lane - 1) << 2;
    const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)(uint32_t)x);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)(uint32_t)((uint64_t)x >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
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

// The lane's parameters (param order of include/bt.h) and what follows from them.
template <int STRAT>
struct LaneParams {
    int32_t w1 = 1, w2 = 1;          // SMA f, s; EMA+OLS span n, window w; Bollinger w (w1)
    int32_t sl_bps = 0, tp_bps = 0;
    int64_t kn = 0;
    int32_t warm;
    double alpha, lo_mult, hi_mult;
    i128 kd2, kn2;
    __device__ __forceinline__ LaneParams(const Grid& g, int32_t param) {
        if (STRAT == BT_BOLL) {
            int32_t p = param;
            tp_bps = g.d[p % g.nd];
            p /= g.nd;
            sl_bps = g.c[p % g.nc];
            p /= g.nc;
            kn = g.b[p % g.nb];
            w1 = g.a[p / g.nb];
        } else {
            w1 = g.a[param / g.nb];
            w2 = g.b[param % g.nb];
        }
        warm = STRAT == BT_BOLL ? w1 - 1 : (w1 > w2 ? w1 : w2) - 1;
        alpha = 2.0 / ((double)w1 + 1.0);
        lo_mult = (double)(10000 - g.band_bps);
        hi_mult = (double)(10000 + g.band_bps);
        kd2 = (i128)((int64_t)g.k_den * g.k_den);
        kn2 = (i128)(kn * kn);
    }
};

// State carried across tiles (wave-uniform).
struct WalkState {
    int32_t pos = 0, ebar = 0, ntr = 0;
    int64_t epx = 0, R = 0, sl_lvl = 0, tp_lvl = 0;
    uint64_t hash = 0;
    uint64_t cA = 0, cB = 0;         // window-sum carries (SMA F, L; EMA+OLS S, U; Bollinger Sc)
    i128 cSc2 = 0;                   // Bollinger sum of c^2
    double e_run = 0.0;              // EMA value after the previous tile's last bar
};

// What a tile leaves in each lane (its bar t = t0 + lane), and the tile's exit bars.
struct TileLanes {
    bool valid;                      // t < B
    int32_t c, cp;                   // c_t, c_(t-1) (1 at t = 0)
    int32_t lpos, lprev;             // position after / before the bar
    int64_t lentry, lreal;           // entry price of that position, pnl realized up to the bar
    uint64_t exits;                  // wave-uniform: bit i = a trade closed at bar t0 + i
};

// Walks tile [t0, t0 + 64) of a symbol of B bars (cs, and hs / ls for Bollinger).
// on_trade(i, n, entry_bar, side, entry_px, exit_px) is called, wave-uniformly, for every trade
// that closes: the lane's n-th, at bar t0 + i.
template <int STRAT, class OnTrade>
__device__ __forceinline__ void walk_tile(const LaneParams<STRAT>& P, const Grid& g, WalkState& st,
                                          const int32_t* __restrict__ cs, const int32_t* __restrict__ hs,
                                          const int32_t* __restrict__ ls, int32_t B, int32_t t0, int lane,
                                          TileLanes& o, OnTrade&& on_trade) {
    const int32_t w1 = P.w1, w2 = P.w2;
    const int32_t t = t0 + lane;
    const bool valid = t < B;
    const int32_t c = valid ? cs[t] : 0;
    const int32_t cp = (valid && t >= 1) ? cs[t - 1] : 1;
    const bool dec = valid && t >= P.warm && t <= B - 2;
    const uint64_t last = (B - 1 - t0) < kTile ? 1ull << (B - 1 - t0) : 0ull;
    // the carried state as locals for the length of the tile
    int32_t pos = st.pos, ebar = st.ebar, ntr = st.ntr;
    int64_t epx = st.epx, R = st.R, sl_lvl = st.sl_lvl, tp_lvl = st.tp_lvl;
    uint64_t hash = st.hash, cA = st.cA, cB = st.cB;
    i128 cSc2 = st.cSc2;
    double e_run = st.e_run;

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
            else e_run = e_run + P.alpha * (ci - e_run);
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
        const bool el = lhs < my_e * P.lo_mult && N >= 0;
        const bool es = !el && lhs > my_e * P.hi_mult && N <= 0;
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
        const bool zt = (i128)D * (i128)D * P.kd2 > P.kn2 * Q;
        mA = __ballot(dec && D < 0 && zt);  // flat -> long
        mB = __ballot(dec && D > 0 && zt);  // flat -> short
        mC = __ballot(dec && D >= 0);       // long -> flat at c
        mD = __ballot(dec && D <= 0);       // short -> flat at c
    }

    // ---- the state machine: one iteration per event
    int32_t lpos = pos, lprev = pos;   // position after / before this lane's bar
    int64_t lentry = epx, lreal = R;
    uint64_t exits = 0;
    auto close_trade = [&](int i, int64_t px) {
        R += (int64_t)pos * (px - epx);
        hash += trade_mix_et((uint32_t)ebar, (uint32_t)(t0 + i), pos > 0);
        exits |= 1ull << i;
        on_trade(i, ntr, ebar, pos, epx, px);
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
                sl_lvl = ce * (lg ? 10000 - P.sl_bps : 10000 + P.sl_bps) / 10000;
                tp_lvl = ce * (lg ? 10000 + P.tp_bps : 10000 - P.tp_bps) / 10000;
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
    st.pos = pos, st.ebar = ebar, st.ntr = ntr;
    st.epx = epx, st.R = R, st.sl_lvl = sl_lvl, st.tp_lvl = tp_lvl;
    st.hash = hash, st.cA = cA, st.cB = cB;
    st.cSc2 = cSc2;
    st.e_run = e_run;
    o.valid = valid;
    o.c = c;
    o.cp = cp;
    o.lpos = lpos;
    o.lprev = lprev;
    o.lentry = lentry;
    o.lreal = lreal;
    o.exits = exits;
}

// A tile as LaneWalk::step leaves it: walk_tile's lanes and, of the lane's bar t,
struct LaneTile : TileLanes {
    int64_t E, d;                    // the equity after it, and E_t - E_(t-1) (E_(-1) = 0)
};

// A lane being walked: its parameters, its symbol's columns and the state carried across tiles.
template <int STRAT>
struct LaneWalk {
    const Grid& g;
    const LaneParams<STRAT> P;
    const int32_t *__restrict__ cs, *__restrict__ hs, *__restrict__ ls;   // hs, ls: null unless Bollinger
    const int32_t B, lane;
    WalkState st;
    int64_t e_prev = 0;              // E of the bar before the next tile (E_(-1) = 0)

    __device__ __forceinline__ LaneWalk(const Grid& g, int64_t off, int32_t bars, int32_t param,
                                        const int32_t* __restrict__ high, const int32_t* __restrict__ low,
                                        const int32_t* __restrict__ close, int lane)
        : g(g), P(g, param), cs(close + off), hs(STRAT == BT_BOLL ? high + off : nullptr),
          ls(STRAT == BT_BOLL ? low + off : nullptr), B(bars), lane(lane) {}

    // Walks tile [t0, t0 + 64); on_trade as walk_tile takes it.
    template <class OnTrade>
    __device__ __forceinline__ LaneTile step(int32_t t0, OnTrade&& on_trade) {
        LaneTile o;
        walk_tile<STRAT>(P, g, st, cs, hs, ls, B, t0, lane, o, on_trade);
        o.E = o.lreal + (int64_t)o.lpos * ((int64_t)o.c - o.lentry);
        const int64_t below = lane_below_i64(o.E, lane);   // by every lane: lane 1 reads lane 0
        o.d = o.E - (lane == 0 ? e_prev : below);
        e_prev = lane63_i64(o.E);
        return o;
    }
    __device__ __forceinline__ LaneTile step(int32_t t0) {
        return step(t0, [](int, int32_t, int32_t, int32_t, int64_t, int64_t) {});
    }
};

// The Sharpe terms of the lane's bar t: r1 = pos_(t-1) q_t and r2 = q2_t where a position was held
// into the bar, else 0, and the ballot of those lanes. |q|, q2 <= 2^56 (spec §3): a tile's sums
// of them fit int64.
struct TileReturns {
    int64_t r1, r2;
    uint64_t held;
};
__device__ __forceinline__ TileReturns tile_returns(const TileLanes& o, int32_t t) {
    const bool held = o.valid && t >= 1 && o.lprev != 0;
    int64_t q, q2;
    fixed_ret(o.c, o.cp, q, q2);
    return TileReturns{held ? (int64_t)o.lprev * q : 0, held ? q2 : 0, __ballot(held)};
}

// Running peak of the equity and the largest drawdown from it (wave-uniform), advanced a tile at
// a time over the lanes `in`: prefix maxima within the tile on top of the carried peak.
struct PeakDrawdown {
    int64_t peak = 0, mdd = 0;
    __device__ __forceinline__ void add(int64_t E, bool in, int lane) {
        const int64_t pm = wave_maxscan_i64(in ? E : INT64_MIN, lane);
        const int64_t pk = pm > peak ? pm : peak;
        const int64_t dd = lane63_i64(wave_maxscan_i64(in ? pk - E : 0, lane));
        mdd = dd > mdd ? dd : mdd;
        peak = lane63_i64(pk);
    }
};

// launch(std::integral_constant<int, BT_...>) for the grid's strategy: the one place that turns
// Grid::strategy into a template argument of a lane kernel.
template <class F>
void launch_by_strategy(int32_t strategy, F&& launch) {
    switch (strategy) {
        case BT_SMA_CROSS: launch(std::integral_constant<int, BT_SMA_CROSS>{}); break;
        case BT_EMA_OLS: launch(std::integral_constant<int, BT_EMA_OLS>{}); break;
        default: launch(std::integral_constant<int, BT_BOLL>{}); break;
    }
}

}  // namespace bt
