// k_boot.hip — the bootstrap reality check on the device (bt_bootstrap / bt_bootstrap_of,
// include/bt.h; semantics: docs/bootstrap_spec.md).
//
// boot_starts_kernel: one thread per (block j, resample b): starts[j][b] = draw j of the counter-form
// SplitMix64 keyed by (seed, b), modulo T; b runs along the threads, so that the 64 resamples of a
// wave load one block index coalesced. The same grid sets vmax to INT64_MIN.
//
// boot_kernel<STRAT, LDS>: one workgroup per lane. Its first wave walks the lane with a LaneWalk
// (walk_tile.h) from tile 0 through the tile of min(to, bars) and writes the exclusive prefix row
// Q[0..T] of the window's increments, Q[k] = E_(from+k-1) - E_(from-1): into dynamic LDS (LDS) or
// into the lane's row of the staging arena. The other waves wait at the barrier. The workgroup then
// repeats the last value over the bars past the row's end and resamples (boot_resample).
//
// boot_prefix_kernel<LDS>: the same for a staged row of increments (bt_bootstrap_of): the first wave
// scans it into Q.
//
// boot_resample: thread = resample b. K steps, each the block's start from the table and
// Q[min(e, T)] - Q[s] (ds_read_b64 on the LDS path); the wrap term Q[e - T] is read under a
// wave-level branch, only in trips (of four steps) where some resample of the wave wraps. The gathers are random:
// two resamples of a 32-lane half meet on a bank pair with probability 1/32 per pair, which the
// hardware serialises; a mirrored row would not change that. Per lane: S_i = Q[T]; n_nonpos, m1 and
// m2 by wave sums of 32-bit limbs (an int128 sum is then nine independent 64-bit sums) and one
// pass over the waves' partials in LDS; S* stored coalesced into boot; S* - S_i folded into
// vmax[g][b] by a 64-bit signed atomic maximum, skipped when a plain load already shows a value at
// least as large (the cell only grows, so a stale load costs an atomic, never a result). Maximum and
// integer sums are order-free: the bits do not depend on scheduling.
//
// boot_finish_kernel: one workgroup per group: best_sum and the lowest lane that reaches it over
// the lanes' records, then n_ge over the group's row of vmax.
#include <algorithm>

#include "plan.h"
#include "walk_tile.h"

namespace bt {

namespace {

__device__ __forceinline__ uint64_t boot_mix(uint64_t seed, uint64_t b, uint64_t k) {
    const uint64_t s0 = seed ^ (b * 0x9E3779B97F4A7C15ULL);
    uint64_t z = s0 + (k + 1) * 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

constexpr int kBootSteps = 4;        // blocks of a resample per trip of the step loop
constexpr int kRedWords = 9;         // m1 and m2 in four 32-bit limbs each, n_nonpos
static_assert((size_t)kBootMaxWaves * kRedWords * 8 <= kBootRedBytes, "the reduction scratch holds every wave's partials");

// The resampling of one lane from its prefix row q[0..T] (LDS or arena), by the whole workgroup.
// `red`: the workgroup's scratch in LDS.
__device__ __forceinline__ void boot_resample(const BootArgs& a, const int64_t* q, const int64_t i, const int32_t g,
                                              uint64_t* red) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nthr = (int)blockDim.x;
    const int32_t T = a.T, B = a.B, K = a.K;
    const int64_t Si = q[T];
    i128 m1 = 0, m2 = 0;
    int64_t nonpos = 0;
    int64_t* vrow = a.vmax + (int64_t)g * B;   // read and updated atomically: not __restrict__
    for (int32_t b0 = tid - lane; b0 < B; b0 += nthr) {   // b0 is wave-uniform: whole waves enter
        const int32_t b = b0 + lane;
        const bool on = b < B;
        const int32_t* __restrict__ sp = a.starts + (on ? b : 0);
        int64_t s_star = 0;
        // kBootSteps blocks per trip: their starts are loaded together, then their prefix values,
        // so that a trip waits for memory once. A step past K has s = len = 0 and adds Q[0] - Q[0].
        for (int32_t j0 = 0; j0 < K; j0 += kBootSteps) {
            int32_t s[kBootSteps], e[kBootSteps];
            bool wrap[kBootSteps], any = false;
#pragma unroll
            for (int u = 0; u < kBootSteps; ++u) {
                const int32_t j = j0 + u;
                const int32_t len = j < K - 1 ? a.Lp : j == K - 1 ? a.last_len : 0;
                s[u] = on && j < K ? sp[(int64_t)j * B] : 0;
                e[u] = s[u] + len;
                wrap[u] = e[u] > T;
                any |= wrap[u];
            }
#pragma unroll
            for (int u = 0; u < kBootSteps; ++u) s_star += q[wrap[u] ? T : e[u]] - q[s[u]];
            if (__ballot(any)) {     // wave-level: some resample of the wave wraps in this trip
#pragma unroll
                for (int u = 0; u < kBootSteps; ++u) s_star += wrap[u] ? q[e[u] - T] : 0;
            }
        }
        if (on) {
            m1 += (i128)s_star;
            m2 += (i128)s_star * (i128)s_star;
            nonpos += s_star <= 0 ? 1 : 0;
            if (a.boot) a.boot[i * B + b] = s_star;
            const int64_t v = s_star - Si;
            if (vrow[b] < v) __hip_atomic_fetch_max(vrow + b, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    // the sums of the workgroup: 32-bit limbs summed apart (no carry between lanes), joined mod 2^128
    const unsigned __int128 u1 = (unsigned __int128)m1, u2 = (unsigned __int128)m2;
    uint64_t w[kRedWords];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        w[k] = (uint64_t)wave_sum_i64((int64_t)(uint64_t)(uint32_t)(u1 >> (32 * k)));
        w[4 + k] = (uint64_t)wave_sum_i64((int64_t)(uint64_t)(uint32_t)(u2 >> (32 * k)));
    }
    w[8] = (uint64_t)wave_sum_i64(nonpos);
    __syncthreads();                 // every wave is done with the scratch's previous use (none) and with q
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kRedWords; ++k) red[wave * kRedWords + k] = w[k];
    }
    __syncthreads();
    if (tid == 0) {
        const int nw = nthr >> 6;
        unsigned __int128 s1 = 0, s2 = 0;
        uint64_t np = 0;
        for (int v = 0; v < nw; ++v) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                s1 += (unsigned __int128)red[v * kRedWords + k] << (32 * k);
                s2 += (unsigned __int128)red[v * kRedWords + 4 + k] << (32 * k);
            }
            np += red[v * kRedWords + 8];
        }
        bt_boot_lane* __restrict__ o = a.rec + i;
        o->sum = Si;
        o->n_nonpos = (int64_t)np;
        o->m1.lo = (uint64_t)s1, o->m1.hi = (int64_t)(uint64_t)(s1 >> 64);
        o->m2.lo = (uint64_t)s2, o->m2.hi = (int64_t)(uint64_t)(s2 >> 64);
    }
}

// q[filled + 1 .. T] = q[filled]: the bars past the row's end add nothing.
__device__ __forceinline__ void boot_fill_tail(int64_t* q, int32_t filled, int32_t T) {
    __syncthreads();
    const int64_t tail = q[filled];
    for (int32_t k = filled + 1 + (int32_t)threadIdx.x; k <= T; k += (int32_t)blockDim.x) q[k] = tail;
    __syncthreads();
}

}  // namespace

__global__ __launch_bounds__(256) void boot_starts_kernel(int32_t* __restrict__ starts, int64_t* __restrict__ vmax,
                                                          const uint64_t seed, const int32_t T, const int32_t B,
                                                          const int64_t n_starts, const int64_t n_vmax) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < n_starts) {
        const int64_t j = idx / B, b = idx - j * B;
        starts[idx] = (int32_t)(boot_mix(seed, (uint64_t)b, (uint64_t)j) % (uint64_t)T);
    }
    if (idx < n_vmax) vmax[idx] = INT64_MIN;
}

// STRAT: bt_strategy; LDS: the prefix row lives in dynamic LDS behind the reduction scratch, else in
// row blockIdx.x of a.rows. Block = 1 to kBootMaxWaves waves; blockIdx.x = the lane of the chunk.
template <int STRAT, bool LDS>
__global__ __launch_bounds__(64 * kBootMaxWaves) void boot_kernel(const BootArgs a, const int32_t* __restrict__ high,
                                                                  const int32_t* __restrict__ low,
                                                                  const int32_t* __restrict__ close, const Grid g) {
    extern __shared__ __align__(16) unsigned char boot_smem[];
    uint64_t* red = reinterpret_cast<uint64_t*>(boot_smem);
    int64_t* q = LDS ? reinterpret_cast<int64_t*>(boot_smem + kBootRedBytes) : a.rows + (int64_t)blockIdx.x * a.pitch;
    const int tid = (int)threadIdx.x;
    const int64_t i = a.lane0 + blockIdx.x;
    LaneRef L;
    int32_t gi;
    if (a.lanes) {
        L = a.lanes[i];
        gi = a.gid[i];
    } else {
        gi = (int32_t)(i / a.P);
        const SymDesc sd = a.syms[gi];
        L = LaneRef{sd.off, sd.bars, (int32_t)(i - (int64_t)gi * a.P)};
    }
    // the lane's bars of the window are [from, end); a row that ends at or before `from` is not walked
    const int64_t to = (int64_t)a.from + a.T;
    const int32_t last = to < (int64_t)L.bars ? (int32_t)to : L.bars;
    const int32_t end = last > a.from ? last : 0;
    const int32_t filled = end > 0 ? end - a.from : 0;   // q[0 .. filled] come from the walk
    if (tid < kTile) {
        LaneWalk<STRAT> lw(g, L.off, L.bars, L.param, high, low, close, tid);
        int64_t base = 0;            // E_(from - 1), wave-uniform
        if (tid == 0) q[0] = 0;
        for (int32_t t0 = 0; t0 < end; t0 += kTile) {
            const LaneTile o = lw.step(t0);
            if (t0 + kTile < a.from) continue;            // before the tile of bar from - 1
            const int32_t bl = a.from - 1 - t0;           // that bar's lane in this tile
            if (bl >= 0 && bl < kTile) base = lane_i64(o.E, bl);
            const int32_t t = t0 + tid;
            if (t >= a.from && t < end) q[t - a.from + 1] = o.E - base;   // t - from + 1 <= filled <= T
        }
    }
    boot_fill_tail(q, filled, a.T);
    boot_resample(a, q, i, gi, red);
}

template <bool LDS>
__global__ __launch_bounds__(64 * kBootMaxWaves) void boot_prefix_kernel(const BootArgs a) {
    extern __shared__ __align__(16) unsigned char boot_smem[];
    uint64_t* red = reinterpret_cast<uint64_t*>(boot_smem);
    int64_t* q = LDS ? reinterpret_cast<int64_t*>(boot_smem + kBootRedBytes) : a.rows + (int64_t)blockIdx.x * a.pitch;
    const int tid = (int)threadIdx.x;
    const int64_t i = a.lane0 + blockIdx.x;
    const int32_t* __restrict__ drow = a.d + (int64_t)blockIdx.x * a.d_pitch;
    if (tid < kTile) {
        int64_t carry = 0;
        if (tid == 0) q[0] = 0;
        for (int32_t k0 = 0; k0 < a.T; k0 += kTile) {
            const int32_t k = k0 + tid;
            const int64_t s = carry + wave_iscan_i64(k < a.T ? (int64_t)drow[k] : 0);
            if (k < a.T) q[k + 1] = s;
            carry = lane63_i64(s);
        }
    }
    __syncthreads();
    boot_resample(a, q, i, a.gid[i], red);
}

constexpr int kFinishThreads = 256;

__global__ __launch_bounds__(kFinishThreads) void boot_finish_kernel(const BootArgs a) {
    __shared__ int64_t sv[kFinishThreads];
    __shared__ int32_t si[kFinishThreads];
    const int tid = (int)threadIdx.x, nthr = (int)blockDim.x;
    const int32_t g = (int32_t)blockIdx.x;
    const int64_t i0 = a.goff ? a.goff[g] : (int64_t)g * a.P, i1 = a.goff ? a.goff[g + 1] : i0 + a.P;
    const int32_t m = (int32_t)(i1 - i0);
    // the largest sum and the lowest lane with it
    int64_t best = INT64_MIN;
    int32_t at = INT32_MAX;
    for (int32_t k = tid; k < m; k += nthr) {
        const int64_t s = a.rec[i0 + k].sum;
        if (s > best) best = s, at = k;   // k rises: of equal sums the first stays
    }
    sv[tid] = best, si[tid] = at;
    __syncthreads();
    for (int h = nthr >> 1; h > 0; h >>= 1) {
        if (tid < h) {
            const int64_t s = sv[tid + h];
            const int32_t k = si[tid + h];
            if (s > sv[tid] || (s == sv[tid] && k < si[tid])) sv[tid] = s, si[tid] = k;
        }
        __syncthreads();
    }
    best = sv[0], at = si[0];
    __syncthreads();
    int64_t n_ge = 0;
    const int64_t* __restrict__ vrow = a.vmax + (int64_t)g * a.B;
    for (int32_t b = tid; b < a.B; b += nthr) n_ge += vrow[b] >= best ? 1 : 0;
    sv[tid] = n_ge;
    __syncthreads();
    for (int h = nthr >> 1; h > 0; h >>= 1) {
        if (tid < h) sv[tid] += sv[tid + h];
        __syncthreads();
    }
    if (tid == 0) {
        bt_boot_group* __restrict__ o = a.groups + g;
        o->best_sum = best;
        o->best_lane = at;
        o->n_lanes = m;
        o->n_ge = sv[0];
    }
}

hipError_t launch_boot_starts(const BootArgs& a, const BootPlan& pl, uint64_t seed, hipStream_t st) {
    const int64_t n_starts = (int64_t)a.K * a.B, n_vmax = (int64_t)a.G * a.B;
    const int64_t blocks = std::max(pl.starts_blocks, (n_vmax + pl.starts_block - 1) / pl.starts_block);
    hipLaunchKernelGGL(boot_starts_kernel, dim3((unsigned)blocks), dim3((unsigned)pl.starts_block), 0, st,
                       const_cast<int32_t*>(a.starts), a.vmax, seed, a.T, a.B, n_starts, n_vmax);
    return hipGetLastError();
}

hipError_t launch_boot_walk(const BootArgs& a, int32_t m, const BootPlan& pl, const int32_t* high, const int32_t* low,
                            const int32_t* close, const Grid& g, hipStream_t st) {
    static_assert(kBootLdsBytes <= 64 * 1024, "dynamic LDS above 64 KB needs hipFuncSetAttribute");
    if (m <= 0) return hipSuccess;
    launch_by_strategy(g.strategy, [&](auto strat) {
        constexpr int S = decltype(strat)::value;
        if (pl.row_mode == 1)
            hipLaunchKernelGGL((boot_kernel<S, true>), dim3((unsigned)m), dim3((unsigned)pl.block), pl.lds_bytes, st, a,
                               high, low, close, g);
        else
            hipLaunchKernelGGL((boot_kernel<S, false>), dim3((unsigned)m), dim3((unsigned)pl.block), pl.lds_bytes, st, a,
                               high, low, close, g);
    });
    return hipGetLastError();
}

hipError_t launch_boot_prefix(const BootArgs& a, int32_t m, const BootPlan& pl, hipStream_t st) {
    if (m <= 0) return hipSuccess;
    if (pl.row_mode == 1)
        hipLaunchKernelGGL(boot_prefix_kernel<true>, dim3((unsigned)m), dim3((unsigned)pl.block), pl.lds_bytes, st, a);
    else
        hipLaunchKernelGGL(boot_prefix_kernel<false>, dim3((unsigned)m), dim3((unsigned)pl.block), pl.lds_bytes, st, a);
    return hipGetLastError();
}

hipError_t launch_boot_finish(const BootArgs& a, const BootPlan& pl, hipStream_t st) {
    static_assert(kFinishThreads == 256, "plan_boot: finish_block is 256, a power of two");
    hipLaunchKernelGGL(boot_finish_kernel, dim3((unsigned)a.G), dim3((unsigned)pl.finish_block), 0, st, a);
    return hipGetLastError();
}

}  // namespace bt
