// k_tail.hip — tail risk on the device: per-lane moments, value at risk and expected shortfall
// (bt_tail / bt_tail_of, include/bt.h; semantics: docs/tail_spec.md).
//
// tail_kernel<STRAT, LDS>: one workgroup of kTailWaves waves per lane. Its first wave walks the lane
// with a LaneWalk (walk_tile.h) from tile 0 through the tile of min(to, bars); the other waves wait
// at the barrier. Per tile tail_add takes the counted lanes' d into the wave's running record
// (TailAcc, wave-uniform): the counts by ballots, the extremes with the first bar that reaches each,
// s1 and s1_neg by wave sums, and the squares, cubes and fourth powers summed in 32-bit limbs (a
// limb's wave sum stays below 2^40) and joined into two int128 and one 192-bit accumulator of three
// 64-bit words with explicit carries. A tile whose counted d are all 0 moves no sum and skips them.
// The counted d go, compacted by a ballot and a prefix popcount onto a carried cursor, as int32
// into the lane's row: dynamic LDS behind the histograms (LDS) or the lane's row of the arena.
//
// tail_of_kernel<LDS>: the same for a staged row of increments (bt_tail_of): the first wave reads it
// in place of the walk; with the arena home the staged row is the row.
//
// tail_select: the whole workgroup, on order-preserving keys (uint32)d ^ 0x80000000. A
// most-significant-digit radix select, four passes of eight bits, every level in the same pass over
// the row: level j counts the keys that share its prefix into its own 256-bin LDS histogram (a wave
// whose hits all fall into one bin adds their count once: rows of mostly equal values would
// otherwise serialise on that bin), then one wave per level scans the bins, four per lane, and the
// lane that owns the k-th key extends the level's prefix and rebases its rank. The levels' prefixes
// live in lane j of one VGPR per wave. After the fourth pass the prefix is var's key; one more pass
// counts and sums the d below each level's var (per-thread registers, wave sums, the waves'
// partials in LDS), and es_sum = that sum + (k - n_lt) var. Counts and integer sums are order-free:
// the bits do not depend on scheduling or on the row's home.
#include "plan.h"
#include "walk_tile.h"

namespace bt {

namespace {

constexpr int kTailThreads = 64 * kTailWaves;
constexpr int kQ = BT_TAIL_LEVELS_MAX;
constexpr uint32_t kKeyFlip = 0x80000000u;

// The workgroup's scratch, behind the histograms.
struct TailShared {
    uint32_t prefix[kQ], rem[kQ];    // per level: the key's digits so far, the rank inside them (1-based)
    int32_t k[kQ];
    int32_t n, pad[7];
    int64_t red_sum[kTailWaves][kQ];
    int32_t red_cnt[kTailWaves][kQ];
};
static_assert(kTailHistBytes + sizeof(TailShared) <= kTailFixedBytes, "the scratch fits in front of the row");
static_assert(kTailHistBytes % 16 == 0 && kTailFixedBytes % 16 == 0, "the scratch and the row are aligned");

__device__ __forceinline__ int32_t wave_min_i32(int32_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const int32_t o = __shfl_xor(v, d, 64);
        v = o < v ? o : v;
    }
    return (int32_t)__builtin_amdgcn_readfirstlane(v);
}
__device__ __forceinline__ int32_t wave_max_i32(int32_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const int32_t o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return (int32_t)__builtin_amdgcn_readfirstlane(v);
}

// A 192-bit unsigned accumulator in three 64-bit words (wave-uniform): v 2^(32 S) is added, v < 2^40.
struct Acc192 {
    uint64_t w0 = 0, w1 = 0, w2 = 0;
    __device__ __forceinline__ void at0(uint64_t v) {
        w0 += v;
        const uint64_t c = w0 < v ? 1 : 0;
        w1 += c;
        w2 += w1 < c ? 1 : 0;
    }
    __device__ __forceinline__ void at1(uint64_t v) {
        w1 += v;
        w2 += w1 < v ? 1 : 0;
    }
    template <int S>
    __device__ __forceinline__ void add(uint64_t v) {
        if (S == 0) at0(v);
        if (S == 1) at0(v << 32), at1(v >> 32);
        if (S == 2) at1(v);
        if (S == 3) at1(v << 32), w2 += v >> 32;
    }
};

// The running record of the wave that walks (wave-uniform).
struct TailAcc {
    int32_t n = 0, n_pos = 0, n_neg = 0, min_bar = -1, max_bar = -1, min_d = 0, max_d = 0;
    int64_t s1 = 0, s1_neg = 0;
    i128 s2 = 0, s2_neg = 0, s3 = 0;
    Acc192 s4;
};

// One tile: the lanes with `counted` add their d (|d| < 2^31), the bar of lane 0 being t0. STORE: the
// counted d go to row[n ..], in lane order.
template <bool STORE>
__device__ __forceinline__ void tail_add(TailAcc& A, int32_t* row, int32_t d, bool counted, int32_t t0, int lane) {
    const uint64_t cm = __ballot(counted);
    if (!cm) return;
    if (STORE && counted) row[A.n + __popcll(cm & ((1ull << lane) - 1ull))] = d;
    d = counted ? d : 0;
    const uint64_t pm = __ballot(d > 0), nm = __ballot(d < 0);
    int32_t mn = 0, mx = 0;          // of the counted lanes: 0 when none of them moved
    if (pm | nm) {
        mn = wave_min_i32(counted ? d : INT32_MAX);
        mx = wave_max_i32(counted ? d : INT32_MIN);
    }
    if (A.n == 0 || mn < A.min_d) {  // strictly: of equal extremes the first bar stays
        A.min_d = mn;
        A.min_bar = t0 + __builtin_ctzll(__ballot(counted && d == mn));
    }
    if (A.n == 0 || mx > A.max_d) {
        A.max_d = mx;
        A.max_bar = t0 + __builtin_ctzll(__ballot(counted && d == mx));
    }
    A.n += __popcll(cm);
    A.n_pos += __popcll(pm);
    A.n_neg += __popcll(nm);
    if (!(pm | nm)) return;          // zeros only: no sum moves

    constexpr uint64_t M = 0xFFFFFFFFull;
    const i128 B32 = (i128)1 << 32, B64 = (i128)1 << 64;
    A.s1 += wave_sum_i64((int64_t)d);
    const uint64_t a = (uint64_t)(uint32_t)(d < 0 ? -d : d);   // < 2^31
    const uint64_t a2 = a * a, h = a2 >> 32, l = a2 & M;       // h < 2^30
    A.s2 += (i128)wave_sum_i64((int64_t)h) * B32 + (i128)wave_sum_i64((int64_t)l);
    // d^3 = sign (l a + (h a) 2^32) in three limbs of at most 33 bits
    const uint64_t p0 = l * a, p1 = h * a;
    const int64_t sg = d < 0 ? -1 : 1;
    const int64_t c0 = sg * (int64_t)(p0 & M), c1 = sg * (int64_t)((p0 >> 32) + (p1 & M)), c2 = sg * (int64_t)(p1 >> 32);
    A.s3 += (i128)wave_sum_i64(c0) + (i128)wave_sum_i64(c1) * B32 + (i128)wave_sum_i64(c2) * B64;
    // d^4 = l l + 2 h l 2^32 + h h 2^64 in four limbs of at most 34 bits
    const uint64_t ll = l * l, hl = h * l, hh = h * h;
    A.s4.add<0>((uint64_t)wave_sum_i64((int64_t)(ll & M)));
    A.s4.add<1>((uint64_t)wave_sum_i64((int64_t)((ll >> 32) + 2 * (hl & M))));
    A.s4.add<2>((uint64_t)wave_sum_i64((int64_t)(2 * (hl >> 32) + (hh & M))));
    A.s4.add<3>((uint64_t)wave_sum_i64((int64_t)(hh >> 32)));
    if (nm) {
        const bool ng = d < 0;
        A.s1_neg += wave_sum_i64(ng ? (int64_t)d : 0);
        A.s2_neg += (i128)wave_sum_i64(ng ? (int64_t)h : 0) * B32 + (i128)wave_sum_i64(ng ? (int64_t)l : 0);
    }
}

// Lane 0 of the first wave: the record, field by field, and n for the selection.
__device__ __forceinline__ void tail_put(const TailArgs& a, const TailAcc& A, int32_t n_window, TailShared* sh) {
    sh->n = A.n;
    if (!a.rec) return;
    bt_tail_rec* __restrict__ o = a.rec + blockIdx.x;
    o->n = A.n;
    o->n_window = n_window;
    o->n_pos = A.n_pos;
    o->n_neg = A.n_neg;
    o->min_bar = A.min_bar;
    o->max_bar = A.max_bar;
    o->min_d = A.min_d;
    o->max_d = A.max_d;
    o->s1 = A.s1;
    o->s1_neg = A.s1_neg;
    o->s2.lo = wide_lo(A.s2), o->s2.hi = wide_hi(A.s2);
    o->s2_neg.lo = wide_lo(A.s2_neg), o->s2_neg.hi = wide_hi(A.s2_neg);
    o->s3.lo = wide_lo(A.s3), o->s3.hi = wide_hi(A.s3);
    o->s4[0] = A.s4.w0, o->s4[1] = A.s4.w1, o->s4[2] = A.s4.w2;
}

// The order statistics of row[0 .. n) at every level, by the whole workgroup, after the barrier that
// ends the first wave's writes.
__device__ __forceinline__ void tail_select(const TailArgs& a, const int32_t* row, TailShared* sh, uint32_t* hist) {
    if (!a.q) return;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t Q = a.Q, n = sh->n;
    bt_tail_q* __restrict__ qo = a.q + (int64_t)blockIdx.x * Q;
    if (n == 0) {
        if (tid < Q) qo[tid].var = 0, qo[tid].es_sum = 0, qo[tid].k = 0, qo[tid].n_lt = 0;
        return;
    }
    if (tid < Q) {
        const int32_t k = (int32_t)(((uint64_t)n * (uint64_t)a.levels[tid] + 999999ull) / 1000000ull);   // in [1, n]
        sh->k[tid] = k;
        sh->rem[tid] = (uint32_t)k;
        sh->prefix[tid] = 0;
    }
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        for (int i = tid; i < Q * 256; i += kTailThreads) hist[i] = 0;
        __syncthreads();             // the histograms are clear, the levels' state of the pass before is written
        const uint32_t vpre = sh->prefix[lane & (kQ - 1)];   // level j's prefix in lane j
        for (int32_t i0 = wave * 64; i0 < n; i0 += kTailThreads) {   // i0 is wave-uniform: whole waves enter
            const int32_t i = i0 + lane;
            const bool on = i < n;
            const uint32_t key = on ? (uint32_t)row[i] ^ kKeyFlip : 0u;
            const uint32_t bin = (key >> shift) & 255u;
            for (int j = 0; j < Q; ++j) {
                const uint32_t pre = (uint32_t)lane_i32((int32_t)vpre, j);
                const bool hit = on && ((uint64_t)(key ^ pre) >> (shift + 8)) == 0;   // the digits above agree
                const uint64_t hm = __ballot(hit);
                if (!hm) continue;
                const int first = __builtin_ctzll(hm);
                const uint32_t b0 = (uint32_t)lane_i32((int32_t)bin, first);
                if (__ballot(hit && bin == b0) == hm) {
                    if (lane == first) atomicAdd(&hist[j * 256 + b0], (uint32_t)__popcll(hm));
                } else if (hit) {
                    atomicAdd(&hist[j * 256 + bin], 1u);
                }
            }
        }
        __syncthreads();
        for (int j = wave; j < Q; j += kTailWaves) {   // a wave per level, four bins per lane
            const uint32_t* hj = hist + j * 256 + 4 * lane;
            const uint32_t c0 = hj[0], c1 = hj[1], c2 = hj[2], c3 = hj[3];
            const uint32_t tot = c0 + c1 + c2 + c3;
            const uint32_t incl = wave_iscan_u32(tot);
            const uint32_t rem = sh->rem[j];
            uint32_t before = incl - tot;
            if (before < rem && rem <= incl) {         // one lane: the k-th key is in its bins
                uint32_t b = 0;
                if (rem > before + c0) {
                    before += c0, b = 1;
                    if (rem > before + c1) {
                        before += c1, b = 2;
                        if (rem > before + c2) before += c2, b = 3;
                    }
                }
                sh->prefix[j] |= (uint32_t)(4 * lane + b) << shift;
                sh->rem[j] = rem - before;
            }
        }
        __syncthreads();
    }
    // the d below each level's var
    const uint32_t vkey = sh->prefix[lane & (kQ - 1)];
    int64_t sl[kQ];
    int32_t cl[kQ];
#pragma unroll
    for (int j = 0; j < kQ; ++j) sl[j] = 0, cl[j] = 0;
    for (int32_t i0 = wave * 64; i0 < n; i0 += kTailThreads) {
        const int32_t i = i0 + lane;
        const bool on = i < n;
        const int32_t d = on ? row[i] : 0;
        const uint32_t key = (uint32_t)d ^ kKeyFlip;
#pragma unroll
        for (int j = 0; j < kQ; ++j) {
            if (j < Q) {
                const bool lt = on && key < (uint32_t)lane_i32((int32_t)vkey, j);
                sl[j] += lt ? (int64_t)d : 0;
                cl[j] += lt ? 1 : 0;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < kQ; ++j) {
        if (j < Q) {
            const int64_t s = wave_sum_i64(sl[j]), c = wave_sum_i64((int64_t)cl[j]);
            if (lane == 0) sh->red_sum[wave][j] = s, sh->red_cnt[wave][j] = (int32_t)c;
        }
    }
    __syncthreads();
    if (tid < Q) {
        int64_t s = 0;
        int32_t c = 0;
        for (int w = 0; w < kTailWaves; ++w) s += sh->red_sum[w][tid], c += sh->red_cnt[w][tid];
        const int64_t var = (int64_t)(int32_t)(sh->prefix[tid] ^ kKeyFlip);
        const int32_t k = sh->k[tid];
        qo[tid].var = var;
        qo[tid].es_sum = s + (int64_t)(k - c) * var;
        qo[tid].k = k;
        qo[tid].n_lt = c;
    }
}

}  // namespace

// STRAT: bt_strategy; LDS: the row lives in dynamic LDS behind kTailFixedBytes, else in row
// blockIdx.x of a.rows. blockIdx.x = the request's index (list mode) or row * P + param of the chunk.
template <int STRAT, bool LDS>
__global__ __launch_bounds__(kTailThreads) void tail_kernel(const TailArgs a, const int32_t* __restrict__ high,
                                                            const int32_t* __restrict__ low,
                                                            const int32_t* __restrict__ close, const Grid g) {
    extern __shared__ __align__(16) unsigned char tail_smem[];
    uint32_t* hist = reinterpret_cast<uint32_t*>(tail_smem);
    TailShared* sh = reinterpret_cast<TailShared*>(tail_smem + kTailHistBytes);
    int32_t* row = LDS ? reinterpret_cast<int32_t*>(tail_smem + kTailFixedBytes) : a.rows + (int64_t)blockIdx.x * a.pitch;
    const int tid = (int)threadIdx.x;
    if (tid < kTile) {
        LaneRef L;
        if (a.lanes) {
            L = a.lanes[blockIdx.x];
        } else {
            const SymDesc sd = a.syms[blockIdx.x / (uint32_t)a.P];
            L = LaneRef{sd.off, sd.bars, (int32_t)(blockIdx.x % (uint32_t)a.P)};
        }
        // the lane's bars of the window are [from, end), never more than the row holds
        int32_t end = a.to < L.bars ? a.to : L.bars;
        if ((int64_t)end - a.from > a.cap) end = a.from + a.cap;
        if (end <= a.from) end = 0;  // a row that ends at or before `from` is not walked
        TailAcc A;
        LaneWalk<STRAT> lw(g, L.off, L.bars, L.param, high, low, close, tid);
        for (int32_t t0 = 0; t0 < end; t0 += kTile) {
            const LaneTile o = lw.step(t0);
            if (t0 + kTile <= a.from) continue;
            const int32_t t = t0 + tid;
            const bool in = t >= a.from && t < end;
            const bool counted = in && (!a.held || (t >= 1 && o.lprev != 0));
            tail_add<true>(A, row, (int32_t)o.d, counted, t0, tid);
        }
        if (tid == 0) tail_put(a, A, end > 0 ? end - a.from : 0, sh);
    }
    __syncthreads();
    tail_select(a, row, sh, hist);
}

template <bool LDS>
__global__ __launch_bounds__(kTailThreads) void tail_of_kernel(const TailArgs a) {
    extern __shared__ __align__(16) unsigned char tail_smem[];
    uint32_t* hist = reinterpret_cast<uint32_t*>(tail_smem);
    TailShared* sh = reinterpret_cast<TailShared*>(tail_smem + kTailHistBytes);
    int32_t* src = a.rows + (int64_t)blockIdx.x * a.pitch;
    int32_t* row = LDS ? reinterpret_cast<int32_t*>(tail_smem + kTailFixedBytes) : src;
    const int tid = (int)threadIdx.x;
    const int32_t T = a.T < a.cap ? a.T : a.cap;
    if (tid < kTile) {
        TailAcc A;
        for (int32_t k0 = 0; k0 < T; k0 += kTile) {
            const int32_t k = k0 + tid;
            const bool in = k < T;
            tail_add<LDS>(A, row, in ? src[k] : 0, in, k0, tid);
        }
        if (tid == 0) tail_put(a, A, T, sh);
    }
    __syncthreads();
    tail_select(a, row, sh, hist);
}

hipError_t launch_tail_walk(const TailArgs& a, int32_t m, const TailPlan& pl, const int32_t* high, const int32_t* low,
                            const int32_t* close, const Grid& g, hipStream_t st) {
    static_assert(kTailLdsBytes <= 64 * 1024, "dynamic LDS above 64 KB needs hipFuncSetAttribute");
    if (m <= 0) return hipSuccess;
    launch_by_strategy(g.strategy, [&](auto strat) {
        constexpr int S = decltype(strat)::value;
        if (pl.row_mode == 1)
            hipLaunchKernelGGL((tail_kernel<S, true>), dim3((unsigned)m), dim3((unsigned)pl.block), pl.lds_bytes, st, a,
                               high, low, close, g);
        else
            hipLaunchKernelGGL((tail_kernel<S, false>), dim3((unsigned)m), dim3((unsigned)pl.block), pl.lds_bytes, st, a,
                               high, low, close, g);
    });
    return hipGetLastError();
}

hipError_t launch_tail_of(const TailArgs& a, int32_t m, const TailPlan& pl, hipStream_t st) {
    if (m <= 0) return hipSuccess;
    if (pl.row_mode == 1)
        hipLaunchKernelGGL(tail_of_kernel<true>, dim3((unsigned)m), dim3((unsigned)pl.block), pl.lds_bytes, st, a);
    else
        hipLaunchKernelGGL(tail_of_kernel<false>, dim3((unsigned)m), dim3((unsigned)pl.block), pl.lds_bytes, st, a);
    return hipGetLastError();
}

}  // namespace bt
