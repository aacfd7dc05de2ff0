// k_portfolio.hip — portfolio of chosen lanes on the device (bt_portfolio, include/bt.h; semantics:
// docs/portfolio_spec.md).
//
// pf_walk_kernel: one wave64 workgroup per entry, a LaneWalk (walk_tile.h) from tile 0 to the tile
// of the window's last bar. The lanes inside the window add their tile's d_t = E_t - E_(t-1) and
// their position, as one packed count word, into the per-bar accumulators with no-return 64-bit
// integer atomics. Integer addition is associative and commutative: the sums do not depend on the
// order in which the waves arrive. No LDS.
//
// pf_finish_kernel: one block over [0, T) in block-wide strips. A thread folds the R replicas of
// its bar and writes pnl, n_long and n_short; the block scans pnl into equity and the equity into
// its running maximum (wave scans, the waves' totals through LDS, the strip's carried on), and
// every thread keeps its own partial drawdown maximum, int128 s1 / s2, gross maximum and exposure,
// reduced once at the end, when thread 0 writes the summary.
#include "plan.h"
#include "walk_tile.h"

namespace bt {

namespace {

__device__ __forceinline__ void add_u64(unsigned long long* p, unsigned long long v) {
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ i128 shfl_down_i128(i128 x, int d) {
    const uint64_t lo = __shfl_down((unsigned long long)wide_lo(x), d, 64);
    const int64_t hi = __shfl_down((long long)wide_hi(x), d, 64);
    return wide_join(lo, hi);
}

}  // namespace

// STRAT: bt_strategy. Block = one wave; blockIdx.x = index of the entry.
template <int STRAT>
__global__ __launch_bounds__(64) void pf_walk_kernel(const PfLane* __restrict__ lanes,
                                                     const int32_t* __restrict__ high,
                                                     const int32_t* __restrict__ low,
                                                     const int32_t* __restrict__ close, const Grid g,
                                                     const PfWork w) {
    const int lane = (int)threadIdx.x;
    const PfLane L = lanes[blockIdx.x];
    LaneWalk<STRAT> lw(g, L.off, L.bars, L.param, high, low, close, lane);
    const int64_t rep = (int64_t)(blockIdx.x % (uint32_t)w.R) * w.pitch;
    unsigned long long* __restrict__ a_pnl = w.acc_pnl + rep;
    unsigned long long* __restrict__ a_cnt = w.acc_cnt + rep;

    // the host clips: from < to <= min(B, T), so every bar added to lies inside a row of T
    for (int32_t t0 = 0; t0 < L.to; t0 += kTile) {
        const int32_t t = t0 + lane;
        const LaneTile o = lw.step(t0);
        if (t0 + kTile <= L.from) continue;   // no atomic before the tile of `from`
        const bool in = t >= L.from && t < L.to;
        const unsigned long long cnt = !in || o.lpos == 0 ? 0ull : o.lpos > 0 ? 1ull : 1ull << 32;
        const bool add_d = in && o.d != 0;
        // warm-up and flat tiles have nothing to add: one wave-uniform test skips both atomics
        if (__ballot(add_d || cnt != 0) == 0) continue;
        if (add_d) add_u64(a_pnl + t, (unsigned long long)o.d);
        if (cnt != 0) add_u64(a_cnt + t, cnt);
    }
}

constexpr int kFinishWaves = 16;     // the finish block is at most this many waves

__global__ __launch_bounds__(kFinishWaves * 64) void pf_finish_kernel(const PfWork w, const double sqrt_ann) {
    // the waves' totals of a strip, double-buffered so that a strip needs two barriers, not three
    __shared__ int64_t s_sum[2][kFinishWaves], s_max[2][kFinishWaves];
    __shared__ int64_t r_mdd[kFinishWaves], r_expo[kFinishWaves];
    __shared__ int32_t r_gross[kFinishWaves];
    __shared__ uint64_t r_s[4][kFinishWaves];
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int nw = (int)(blockDim.x >> 6);
    const int32_t T = w.T;

    int64_t c_eq = 0, c_peak = 0;    // carried across strips (block-uniform): equity, its maximum (>= 0)
    int64_t mdd = 0, expo = 0;       // per thread, reduced at the end
    int32_t gross = 0;
    i128 s1 = 0, s2 = 0;
    int buf = 0;
    for (int32_t b0 = 0; b0 < T; b0 += (int32_t)blockDim.x, buf ^= 1) {
        const int32_t t = b0 + tid;
        const bool live = t < T;
        int64_t p = 0;
        uint64_t cnt = 0;
        if (live)
            for (int32_t r = 0; r < w.R; ++r) {
                p += (int64_t)w.acc_pnl[(int64_t)r * w.pitch + t];
                cnt += w.acc_cnt[(int64_t)r * w.pitch + t];
            }
        const int32_t nl = (int32_t)(uint32_t)cnt, ns = (int32_t)(cnt >> 32);
        if (live) {
            w.pnl[t] = p;
            w.n_long[t] = nl;
            w.n_short[t] = ns;
        }
        gross = max(gross, nl + ns);
        expo += nl + ns;
        // |pnl[t]| < 2^51 (spec §5): the square through the 64 x 64 -> 128 product
        const uint64_t m = (uint64_t)(p < 0 ? -p : p);
        s1 += (i128)p;
        s2 += wide_join(m * m, (int64_t)__umul64hi(m, m));

        // equity: inclusive scan of pnl over the strip, on top of the carry
        const int64_t in_wave = wave_iscan_i64(p);
        if (lane == 63) s_sum[buf][wv] = in_wave;
        __syncthreads();
        int64_t before = c_eq, total = c_eq;
        for (int i = 0; i < nw; ++i) {
            const int64_t x = s_sum[buf][i];
            before += i < wv ? x : 0;
            total += x;
        }
        const int64_t eq = before + in_wave;
        if (live) w.equity[t] = eq;
        // peak: inclusive prefix maximum of the equity (a bar past T repeats the last equity)
        const int64_t mx = wave_maxscan_i64(eq, lane);
        if (lane == 63) s_max[buf][wv] = mx;
        __syncthreads();
        int64_t peak = c_peak, all = c_peak;
        for (int i = 0; i < nw; ++i) {
            const int64_t x = s_max[buf][i];
            peak = i < wv && x > peak ? x : peak;
            all = x > all ? x : all;
        }
        peak = mx > peak ? mx : peak;
        mdd = max(mdd, peak - eq);
        c_eq = total;
        c_peak = all;
    }

    // ---- the threads' partials as one
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        mdd = max(mdd, (int64_t)__shfl_down((long long)mdd, d, 64));
        expo += (int64_t)__shfl_down((long long)expo, d, 64);
        gross = max(gross, __shfl_down(gross, d, 64));
        s1 += shfl_down_i128(s1, d);
        s2 += shfl_down_i128(s2, d);
    }
    if (lane == 0) {
        r_mdd[wv] = mdd;
        r_expo[wv] = expo;
        r_gross[wv] = gross;
        r_s[0][wv] = wide_lo(s1);
        r_s[1][wv] = (uint64_t)wide_hi(s1);
        r_s[2][wv] = wide_lo(s2);
        r_s[3][wv] = (uint64_t)wide_hi(s2);
    }
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < nw; ++i) {
            mdd = max(mdd, r_mdd[i]);
            expo += r_expo[i];
            gross = max(gross, r_gross[i]);
            s1 += wide_join(r_s[0][i], (int64_t)r_s[1][i]);
            s2 += wide_join(r_s[2][i], (int64_t)r_s[3][i]);
        }
        bt_pf_summary* __restrict__ s = w.sum;
        s->n_lanes = w.n_lanes;
        s->first_bar = w.lo;
        s->n_bars = w.hi - w.lo;
        s->max_gross = gross;
        s->pnl = c_eq;
        s->mdd = mdd;
        s->exposure = expo;
        wide_split(s1, s->s1_lo, s->s1_hi);
        wide_split(s2, s->s2_lo, s->s2_hi);
        s->sharpe = sharpe_ticks(s1, s2, w.hi - w.lo, sqrt_ann);
    }
}

hipError_t launch_portfolio(const PfLane* lanes, int32_t n, const int32_t* high, const int32_t* low,
                            const int32_t* close, const Grid& g, const PfWork& w, const PortfolioPlan& pl,
                            hipStream_t st) {
    if (n > 0) {
        launch_by_strategy(g.strategy, [&](auto strat) {
            hipLaunchKernelGGL(pf_walk_kernel<decltype(strat)::value>, dim3((unsigned)n), dim3(kTile), 0, st, lanes,
                               high, low, close, g, w);
        });
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    hipLaunchKernelGGL(pf_finish_kernel, dim3(1), dim3((unsigned)pl.finish_block), 0, st, w, g.sqrt_ann);
    return hipGetLastError();
}

}  // namespace bt
