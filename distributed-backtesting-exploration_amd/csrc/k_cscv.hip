// k_cscv.hip — probability of backtest overfitting on the device (bt_cscv / bt_cscv_of,
// include/bt.h; semantics: docs/cscv_spec.md).
//
// cscv_pack_kernel: one thread per (row, lane) of a chunk: the s1/s2 words of the lane's K fold records as K
// CscvSum, then their total T_p; the thread of lane 0 also leaves the row's K return-bar counts.
//
// cscv_kernel: one thread per combination pair (c, C - 1 - c) of one row (grid y). The thread
// holds the mask M of c and walks the row's lanes twice. For lane p it forms A = sum of the folds
// in M by K masked int128 adds and B = T_p - A, and takes sharpe_fx of both: they are the
// in-sample Sharpe of c and of its complement, and each other's out-of-sample Sharpe. Pass 1 keeps
// the best key and the lowest lane for both directions, with that lane's key on the other half;
// pass 2 counts the lanes below and level with the two winners there. No LDS, no barrier, no
// cross-thread reduction but the wave ballots in front of the group counters' atomics. The fold
// sums are one address for the whole block: they are indexed from kernel arguments, blockIdx and
// the loop counters through const __restrict__ kernel parameters, so they arrive by scalar loads.
#include "plan.h"

namespace bt {

namespace {

struct HalfKeys {
    uint64_t a, b;                 // order keys of the Sharpe over M and over the complement
    bool a_neg, b_neg;             // the halves' s1 below 0
};

// Lane sums sp[0 .. K) and total sp[K]: the two halves under mask M with nA / nB return bars.
__device__ __forceinline__ HalfKeys half_keys(const CscvSum* __restrict__ sp, int32_t K, uint32_t M, int32_t nA,
                                              int32_t nB, double sqrt_ann) {
    i128 a1 = 0, a2 = 0;
#pragma unroll 4
    for (int32_t k = 0; k < K; ++k) {
        const CscvSum f = sp[k];
        const uint64_t m = 0ull - (uint64_t)((M >> k) & 1u);
        a1 += wide_join(f.s1_lo & m, f.s1_hi & (int64_t)m);
        a2 += wide_join(f.s2_lo & m, f.s2_hi & (int64_t)m);
    }
    const CscvSum t = sp[K];
    const i128 b1 = wide_join(t.s1_lo, t.s1_hi) - a1, b2 = wide_join(t.s2_lo, t.s2_hi) - a2;
    HalfKeys h;
    h.a = order_key(sharpe_fx(a1, a2, nA + 1, sqrt_ann));
    h.b = order_key(sharpe_fx(b1, b2, nB + 1, sqrt_ann));
    h.a_neg = a1 < 0;
    h.b_neg = b1 < 0;
    return h;
}

__device__ __forceinline__ double key_sharpe(uint64_t k) {   // order_key back to the double
    union { uint64_t u; double d; } v;
    v.u = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFULL) : ~k;
    return v.d;
}

// One add per wave for a counter both combinations of every thread may bump (no thread leaves
// the kernel early: lane 0 is there).
__device__ __forceinline__ void wave_count(int32_t* dst, bool x, bool y) {
    const int32_t n = (int32_t)(__popcll(__ballot(x)) + __popcll(__ballot(y)));
    if (n && __lane_id() == 0) atomicAdd(dst, n);
}

}  // namespace

__global__ __launch_bounds__(256) void cscv_pack_kernel(const CscvArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // row * P + lane
    if (i >= (int64_t)a.n_rows * a.P) return;
    const int32_t row = (int32_t)(i / a.P), p = (int32_t)(i % a.P), K = a.K;
    const bt_fold* __restrict__ rec = a.rec + (int64_t)row * K * a.P + (int64_t)p * a.stride_p;
    CscvSum* __restrict__ out = a.sums + ((int64_t)row * a.P + p) * (K + 1);
    i128 t1 = 0, t2 = 0;
    for (int32_t k = 0; k < K; ++k) {
        const bt_fold& f = rec[(int64_t)k * a.stride_k];
        out[k] = CscvSum{f.s1_lo, f.s1_hi, f.s2_lo, f.s2_hi};
        t1 += wide_join(f.s1_lo, f.s1_hi);
        t2 += wide_join(f.s2_lo, f.s2_hi);
        if (p == 0) a.nret[(int64_t)row * K + k] = f.n_bars - (f.first_bar == 0 && f.n_bars > 0 ? 1 : 0);
    }
    out[K] = CscvSum{wide_lo(t1), wide_hi(t1), wide_lo(t2), wide_hi(t2)};
}

// Block = pl.block threads along the pairs [q0, q1); blockIdx.y = row - row0.
__global__ __launch_bounds__(256) void cscv_kernel(const CscvArgs a, const CscvSum* __restrict__ sums,
                                                   const int32_t* __restrict__ nret,
                                                   const uint32_t* __restrict__ masks, const int32_t row0,
                                                   const int64_t q0, const int64_t q1, const double sqrt_ann) {
    const int32_t row = row0 + (int32_t)blockIdx.y, P = a.P, K = a.K;
    const int64_t q = q0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = q < q1;
    const uint32_t M = active ? masks[q] : 0u;
    const CscvSum* __restrict__ S = sums + (int64_t)row * P * (K + 1);
    const int32_t* __restrict__ nr = nret + (int64_t)row * K;

    int32_t nA = 0, nT = 0;
    for (int32_t k = 0; k < K; ++k) {
        const int32_t n = nr[k];
        nT += n;
        nA += (M >> k) & 1u ? n : 0;
    }
    const int32_t nB = nT - nA;
    const bool live = active && nA > 0 && nB > 0;

    // ---- pass 1: the winners of both directions (A: in-sample = M; B: in-sample = the complement)
    uint64_t bestA = 0, bestB = 0, oosA = 0, oosB = 0;
    int32_t pA = 0, pB = 0, tieA = 0, tieB = 0;
    bool lossA = false, lossB = false;
    for (int32_t p = 0; p < P; ++p) {
        const HalfKeys h = half_keys(S + (int64_t)p * (K + 1), K, M, nA, nB, sqrt_ann);
        if (p == 0 || h.a > bestA) bestA = h.a, pA = p, tieA = 0, oosA = h.b, lossA = h.b_neg;
        else if (h.a == bestA) ++tieA;
        if (p == 0 || h.b > bestB) bestB = h.b, pB = p, tieB = 0, oosB = h.a, lossB = h.a_neg;
        else if (h.b == bestB) ++tieB;
    }
    // ---- pass 2: the winners' ranks on the other half
    int32_t belowA = 0, equalA = 0, belowB = 0, equalB = 0;
    for (int32_t p = 0; p < P; ++p) {
        const HalfKeys h = half_keys(S + (int64_t)p * (K + 1), K, M, nA, nB, sqrt_ann);
        belowA += h.b < oosA;
        equalA += h.b == oosA && p != pA;
        belowB += h.a < oosB;
        equalB += h.a == oosB && p != pB;
    }
    const int32_t r2A = 2 * belowA + equalA, r2B = 2 * belowB + equalB;

    bt_cscv_group* __restrict__ grp = a.groups + row;
    wave_count(&grp->n_live, live, live);
    wave_count(&grp->n_dead, active && !live, active && !live);
    wave_count(&grp->n_overfit, live && r2A <= P - 1, live && r2B <= P - 1);
    wave_count(&grp->n_loss, live && lossA, live && lossB);
    wave_count(&grp->n_tied, live && tieA > 0, live && tieB > 0);
    if (a.hist && live) {
        uint32_t* __restrict__ h = a.hist + (int64_t)row * (2 * (int64_t)P - 1);
        atomicAdd(h + r2A, 1u);
        atomicAdd(h + r2B, 1u);
    }
    if (a.picks && active) {
        bt_cscv_pick* pk = a.picks + (int64_t)row * a.C;
        bt_cscv_pick* x = pk + q;
        bt_cscv_pick* y = pk + (a.C - 1 - q);
        x->lane = live ? pA : -1;
        x->r2 = live ? r2A : 0;
        x->is_sharpe = live ? key_sharpe(bestA) : 0.0;
        x->oos_sharpe = live ? key_sharpe(oosA) : 0.0;
        y->lane = live ? pB : -1;
        y->r2 = live ? r2B : 0;
        y->is_sharpe = live ? key_sharpe(bestB) : 0.0;
        y->oos_sharpe = live ? key_sharpe(oosB) : 0.0;
    }
}

hipError_t launch_cscv_pack(const CscvArgs& a, const CscvPlan& pl, hipStream_t st) {
    if (a.n_rows <= 0) return hipSuccess;
    const dim3 grid((unsigned)(((int64_t)a.n_rows * a.P + pl.pack_block - 1) / pl.pack_block)), block((unsigned)pl.pack_block);
    hipLaunchKernelGGL(cscv_pack_kernel, grid, block, 0, st, a);
    return hipGetLastError();
}

hipError_t launch_cscv(const CscvArgs& a, const CscvPlan& pl, int32_t row0, int32_t rows, int64_t q0, int64_t q1,
                       double sqrt_ann, hipStream_t st) {
    if (rows <= 0 || q1 <= q0) return hipSuccess;
    const dim3 grid((unsigned)((q1 - q0 + pl.block - 1) / pl.block), (unsigned)rows), block((unsigned)pl.block);
    hipLaunchKernelGGL(cscv_kernel, grid, block, 0, st, a, a.sums, a.nret, a.masks, row0, q0, q1, sqrt_ann);
    return hipGetLastError();
}

}  // namespace bt
