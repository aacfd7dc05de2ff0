// k_walkfwd.hip — walk-forward evaluation on the device (bt_walk_forward, include/bt.h; semantics:
// docs/walkforward_spec.md).
//
// wf_walk_kernel: every (row, param) lane of a chunk of dataset rows, one wave64 workgroup each,
// a LaneWalk (walk_tile.h) over its whole series. On top of a tile's per-lane E_t and
// tile_returns the fold accounting is wave-uniform: for each fold that meets the tile (usually
// one) a lane mask selects its bars, the Sharpe sums are tile partials in int64 added to int128,
// exposure and closed trades are popcounts of ballots under the mask, and the fold-local peak and
// drawdown are a PeakDrawdown under the mask restarted at E(c_k), which is read by readlane at the
// boundary or carried from the previous tile. Lane 0 writes a fold's record when its last bar has
// passed. No LDS.
//
// wf_select_kernel: one workgroup per (row, step), threads striding over p: each sums its lane's
// S1/S2 over the training folds in int128, takes sharpe_fx of them, and the block reduces to the
// largest Sharpe, ties to the lowest param (the order of bt_surface's best); one thread writes
// the step with the winner's record of the out-of-sample fold.
#include "plan.h"
#include "walk_tile.h"

namespace bt {

namespace {

// return bars of fold [ck, ck1): t in [max(ck, 1), ck1)
__device__ __forceinline__ int32_t fold_n_ret(int32_t ck, int32_t ck1) {
    const int32_t a = ck > 1 ? ck : 1;
    return ck1 > a ? ck1 - a : 0;
}

}  // namespace

// STRAT: bt_strategy. Block = one wave; blockIdx.x = row * P + param.
template <int STRAT>
__global__ __launch_bounds__(64) void wf_walk_kernel(const WfArgs a, const int32_t* __restrict__ high,
                                                     const int32_t* __restrict__ low,
                                                     const int32_t* __restrict__ close, const Grid g) {
    const int lane = (int)threadIdx.x;
    const int32_t row = (int32_t)(blockIdx.x / (uint32_t)a.P), param = (int32_t)(blockIdx.x % (uint32_t)a.P);
    const SymDesc sd = a.syms[row];
    const LaneRef L{sd.off, sd.bars, param};
    const int32_t B = L.bars, K = a.K;
    const int32_t* __restrict__ bnd = a.bounds;
    bt_fold* __restrict__ rec = a.rec + ((int64_t)row * K) * a.P + param;   // fold k at rec[k * P]
    LaneWalk<STRAT> lw(g, L.off, L.bars, L.param, high, low, close, lane);

    // empty folds: the staging is zero, only first_bar = c_k is theirs
    for (int32_t k = lane; k < K; k += kTile) {
        const int32_t ck = min(bnd[k], B), ck1 = min(bnd[k + 1], B);
        if (ck1 <= ck) rec[(int64_t)k * a.P].first_bar = ck;
    }

    // ---- carried across tiles (wave-uniform): the open fold k and its sums
    int32_t k = 0, f_expo = 0, f_ntr = 0;
    int64_t f_base = 0;
    PeakDrawdown f_pd;
    i128 f_s1 = 0, f_s2 = 0;

    for (int32_t t0 = 0; t0 < B && k < K; t0 += kTile) {
        const int64_t e_prev = lw.e_prev;        // E of the bar before the tile: E(t0)
        const LaneTile w = lw.step(t0);
        const TileReturns ret = tile_returns(w, t0 + lane);
        const int32_t t1 = min(t0 + kTile, B);   // the tile holds bars [t0, t1)

        while (k < K) {
            const int32_t ck = min(bnd[k], B), ck1 = min(bnd[k + 1], B);
            if (ck1 <= ck) {         // empty: written above
                ++k;
                continue;
            }
            if (ck >= t1) break;     // starts in a later tile
            if (ck >= t0) {          // starts here: E(c_k) is the bar before it
                f_base = ck == t0 ? e_prev : lane_i64(w.E, ck - t0 - 1);
                f_pd = PeakDrawdown{f_base, 0};
                f_expo = f_ntr = 0;
                f_s1 = f_s2 = 0;
            }
            const int lo = max(ck - t0, 0), hi = min(ck1, t1) - t0;   // its lanes [lo, hi)
            const uint64_t mask = from_bit(lo) & ~from_bit(hi);
            const bool in = (mask >> lane) & 1;
            f_s1 += (i128)wave_sum_i64(in ? ret.r1 : 0);
            f_s2 += (i128)wave_sum_i64(in ? ret.r2 : 0);
            f_expo += __popcll(ret.held & mask);
            f_ntr += __popcll(w.exits & mask);
            f_pd.add(w.E, in, lane);
            if (ck1 > t1) break;     // goes on in the next tile
            const int64_t e_end = lane_i64(w.E, ck1 - 1 - t0);
            if (lane == 0) {
                bt_fold f;
                f.first_bar = ck;
                f.n_bars = ck1 - ck;
                f.n_trades = f_ntr;
                f.status = 0;
                f.pnl = e_end - f_base;
                f.mdd = f_pd.mdd;
                f.exposure = f_expo;
                wide_split(f_s1, f.s1_lo, f.s1_hi);
                wide_split(f_s2, f.s2_lo, f.s2_hi);
                f.sharpe = sharpe_fx(f_s1, f_s2, fold_n_ret(ck, ck1) + 1, g.sqrt_ann);
                rec[(int64_t)k * a.P] = f;
            }
            ++k;
        }
    }
}

constexpr int kSelWaves = 4;         // the selection block is at most this many waves

__global__ __launch_bounds__(kSelWaves * 64) void wf_select_kernel(const WfArgs a, const double sqrt_ann) {
    __shared__ uint64_t s_key[kSelWaves];
    __shared__ int32_t s_p[kSelWaves];
    const int tid = (int)threadIdx.x;
    const int32_t row = (int32_t)(blockIdx.x / (uint32_t)a.n_steps);
    const int32_t j = a.j0 + (int32_t)(blockIdx.x % (uint32_t)a.n_steps);
    const int32_t B = a.syms[row].bars, K = a.K, P = a.P;
    const int32_t f0 = a.train == 0 ? 0 : j - a.train;
    int32_t n = 0;                   // return bars of the training window
    for (int32_t k = f0; k < j; ++k) n += fold_n_ret(min(a.bounds[k], B), min(a.bounds[k + 1], B));
    const int32_t cj = min(a.bounds[j], B), cj1 = min(a.bounds[j + 1], B);
    const bool live = n > 0 && cj1 > cj;
    const bt_fold* __restrict__ rec = a.rec + (int64_t)row * K * P;

    uint64_t bk = 0;
    int32_t bp = INT32_MAX;
    if (live)
        for (int32_t p = tid; p < P; p += (int32_t)blockDim.x) {
            i128 s1 = 0, s2 = 0;
            for (int32_t k = f0; k < j; ++k) {
                const bt_fold& r = rec[(int64_t)k * P + p];
                s1 += wide_join(r.s1_lo, r.s1_hi);
                s2 += wide_join(r.s2_lo, r.s2_hi);
            }
            const uint64_t key = order_key(sharpe_fx(s1, s2, n + 1, sqrt_ann));
            if (key > bk || (key == bk && p < bp)) bk = key, bp = p;
        }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint64_t ok = __shfl_down((unsigned long long)bk, d, 64);
        const int32_t op = __shfl_down(bp, d, 64);
        if (ok > bk || (ok == bk && op < bp)) bk = ok, bp = op;
    }
    if ((tid & 63) == 0) s_key[tid >> 6] = bk, s_p[tid >> 6] = bp;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w)
            if (s_key[w] > bk || (s_key[w] == bk && s_p[w] < bp)) bk = s_key[w], bp = s_p[w];
        // field by field into global memory: no private copy of the 104-byte record
        bt_wf_step* __restrict__ s = a.steps + ((int64_t)row * a.n_steps + (j - a.j0));
        s->sym = a.syms[row].id;
        s->fold = j;
        s->param = live ? bp : -1;
        s->pad = 0;
        union { uint64_t u; double d; } v;   // order_key back to the double
        v.u = (bk >> 63) ? (bk & 0x7FFFFFFFFFFFFFFFULL) : ~bk;
        s->train_sharpe = live ? v.d : 0.0;
        const uint64_t* __restrict__ src = reinterpret_cast<const uint64_t*>(rec + ((int64_t)j * P + (live ? bp : 0)));
        uint64_t* __restrict__ dst = reinterpret_cast<uint64_t*>(&s->oos);
        static_assert(sizeof(bt_fold) == 80 && offsetof(bt_fold, n_bars) == 4, "bt_fold as ten words");
#pragma unroll
        for (int i = 0; i < 10; ++i) dst[i] = live ? src[i] : (i == 0 ? (uint64_t)(uint32_t)cj : 0ull);
    }
}

hipError_t launch_wf_walk(const WfArgs& a, const int32_t* high, const int32_t* low, const int32_t* close,
                          const Grid& g, hipStream_t st) {
    if (a.n_rows <= 0) return hipSuccess;
    launch_by_strategy(g.strategy, [&](auto strat) {
        hipLaunchKernelGGL(wf_walk_kernel<decltype(strat)::value>, dim3((unsigned)((int64_t)a.n_rows * a.P)),
                           dim3(kTile), 0, st, a, high, low, close, g);
    });
    return hipGetLastError();
}

hipError_t launch_wf_select(const WfArgs& a, const Grid& g, const WalkfwdPlan& pl, hipStream_t st) {
    if (a.n_rows <= 0 || a.n_steps <= 0) return hipSuccess;
    const dim3 grid((unsigned)((int64_t)a.n_rows * a.n_steps)), block((unsigned)pl.sel_block);
    hipLaunchKernelGGL(wf_select_kernel, grid, block, 0, st, a, g.sqrt_ann);
    return hipGetLastError();
}

}  // namespace bt
