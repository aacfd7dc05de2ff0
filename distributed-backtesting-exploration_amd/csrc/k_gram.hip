// k_gram.hip — covariance of chosen lanes on the device (bt_covariance, bt_gram_of, include/bt.h;
// semantics: docs/covariance_spec.md).
//
// gram_walk_kernel: one wave64 workgroup per lane, a LaneWalk (walk_tile.h) from tile 0 to the tile
// of the window's last bar. The lanes inside the window store their tile's d_t = E_t - E_(t-1) as
// int32 into row i of D at column t - from. The row sum is a carried wave sum, written once. No LDS.
//
// gram_mfma_kernel: D * D^T on v_mfma_f64_16x16x4_f64, one wave per 16 x 16 tile (I <= J) and bar
// chunk. Every increment is split into two signed 16-bit halves,
//     l = ((d + 2^15) & 0xFFFF) - 2^15   (in unsigned words: d + 2^15 leaves int32),
//     h = (d - l) / 2^16,                 d = h * 2^16 + l,
// with |l| <= 2^15 and, for |d| < 2^31, |h| <= 2^15 (d = 0x7FFF8000 gives h = 2^15, l = -2^15), so
//     d_i d_j = h_i h_j * 2^32 + (h_i l_j + l_i h_j) * 2^16 + l_i l_j.
// The exactness bound: every product of two halves is an integer of magnitude <= 2^30, which a
// double holds exactly; a window has at most 2^22 bars, so every partial sum of such products, in
// whatever order the matrix core adds the four k-steps of an instruction and the instructions
// follow each other, is an integer of magnitude <= 2^22 * 2^30 = 2^52 < 2^53 and is held exactly
// too. Each of the four accumulators HH, HL, LH, LL is therefore an exact integer at every step:
// no rounding occurs anywhere and no flush is needed at any legal T. (HL and LH are kept apart;
// together they would reach 2^53 exactly at h = 2^15, l = -2^15 over 2^22 bars.) At the end of its
// chunk a wave converts the accumulators to int64 (exact) and writes HH * 2^32 + (HL + LH) * 2^16
// + LL as one int128 per element, |.| <= 2^84 + 2^70 + 2^52.
// Operands: the sum over k is order-free, so lane (r = lane & 15, q = lane >> 4) loads 16
// contiguous bytes, the bars [16 g + 4 q, 16 g + 4 q + 4) of row 16 I + r (A) and of row 16 J + r
// (B), and feeds element e in k-step e of group g: A and B use the same map, k-slot q of step e is
// bar 16 g + 4 q + e in both. The result uses the f64 C/D map: col = lane & 15,
// row = (lane >> 4) + 4 * reg.
//
// gram_fold_kernel: one thread per element of gram[n][n] adds the chunk partials in int128, the
// lower triangle reading the mirrored element; for a staged D (bt_gram_of) n more blocks sum one
// row of D each.
#include "plan.h"
#include "walk_tile.h"

namespace bt {

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void split16(int32_t d, double& h, double& l) {
    const int32_t lo = (int32_t)(((uint32_t)d + 0x8000u) & 0xFFFFu) - 0x8000;
    // (d - lo) / 2^16 without the 64-bit difference: d >> 16 rounds down, and lo < 0 is the carry
    const int32_t hi = (d >> 16) + (int32_t)((uint32_t)lo >> 31);
    h = (double)hi;
    l = (double)lo;
}

}  // namespace

// STRAT: bt_strategy. Block = one wave; blockIdx.x = the lane's row of D.
template <int STRAT>
__global__ __launch_bounds__(64) void gram_walk_kernel(const LaneRef* __restrict__ lanes,
                                                       const int32_t* __restrict__ high,
                                                       const int32_t* __restrict__ low,
                                                       const int32_t* __restrict__ close, const Grid g,
                                                       const GramWork w, const int32_t from, const int32_t to) {
    const int lane = (int)threadIdx.x;
    const LaneRef L = lanes[blockIdx.x];
    const int32_t last = to < L.bars ? to : L.bars;
    // the lane's bars of the window are [from, end); a symbol that ends before `from` is not walked
    const int32_t end = last > from ? last : 0;
    LaneWalk<STRAT> lw(g, L.off, L.bars, L.param, high, low, close, lane);
    int32_t* __restrict__ row = w.D + (int64_t)blockIdx.x * w.pitch;

    int64_t total = 0;               // the row sum so far (wave-uniform)
    // end <= to <= from + T: every column stored to lies inside a row of T
    for (int32_t t0 = 0; t0 < end; t0 += kTile) {
        const int32_t t = t0 + lane;
        const LaneTile o = lw.step(t0);
        if (t0 + kTile <= from) continue;     // nothing is stored before the tile of `from`
        const bool in = t >= from && t < end;
        if (in) row[t - from] = (int32_t)o.d;   // |d| < 2^31 (docs/portfolio_spec.md §5)
        total += wave_sum_i64(in ? o.d : 0);
    }
    if (lane == 0) w.sums[blockIdx.x] = total;
}

// Block = one wave; blockIdx.x = tile of the upper triangle, blockIdx.y = bar chunk.
__global__ __launch_bounds__(64) void gram_mfma_kernel(const GramWork w) {
    const int lane = (int)threadIdx.x;
    const int r = lane & 15, q = lane >> 4;
    // tile index -> (I, J), I <= J: row I of the triangle holds nt - I tiles
    int I = 0, rem = (int)blockIdx.x;
    while (rem >= w.nt - I) {
        rem -= w.nt - I;
        ++I;
    }
    const int J = I + rem;
    const int32_t ia = 16 * I + r, ib = 16 * J + r;
    // rows past n read the last row and count as zero: no load leaves D, no branch in the loop
    const bool has_a = ia < w.n, has_b = ib < w.n;
    const int32_t* __restrict__ pa = w.D + (int64_t)(has_a ? ia : w.n - 1) * w.pitch + 4 * q;
    const int32_t* __restrict__ pb = w.D + (int64_t)(has_b ? ib : w.n - 1) * w.pitch + 4 * q;
    const int64_t k0 = (int64_t)blockIdx.y * w.chunk_bars;
    const int64_t k1 = k0 + w.chunk_bars < w.pitch ? k0 + w.chunk_bars : w.pitch;   // both multiples of 64

    f64x4 hh = {0, 0, 0, 0}, hl = {0, 0, 0, 0}, lh = {0, 0, 0, 0}, ll = {0, 0, 0, 0};
    // 64 bars per trip: the four groups' loads are issued together, then 64 matrix instructions;
    // the other waves of the SIMD cover the one wait
    for (int64_t k = k0; k < k1; k += 64) {
        int4 a[4], b[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            a[g] = *reinterpret_cast<const int4*>(pa + k + 16 * g);
            b[g] = *reinterpret_cast<const int4*>(pb + k + 16 * g);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int32_t av[4] = {has_a ? a[g].x : 0, has_a ? a[g].y : 0, has_a ? a[g].z : 0, has_a ? a[g].w : 0};
            const int32_t bv[4] = {has_b ? b[g].x : 0, has_b ? b[g].y : 0, has_b ? b[g].z : 0, has_b ? b[g].w : 0};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                double ah, al, bh, bl;
                split16(av[e], ah, al);
                split16(bv[e], bh, bl);
                hh = __builtin_amdgcn_mfma_f64_16x16x4f64(ah, bh, hh, 0, 0, 0);
                hl = __builtin_amdgcn_mfma_f64_16x16x4f64(ah, bl, hl, 0, 0, 0);
                lh = __builtin_amdgcn_mfma_f64_16x16x4f64(al, bh, lh, 0, 0, 0);
                ll = __builtin_amdgcn_mfma_f64_16x16x4f64(al, bl, ll, 0, 0, 0);
            }
        }
    }
    bt_wide* __restrict__ out = w.partial + ((int64_t)blockIdx.y * w.tiles + blockIdx.x) * 256;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const i128 v = (i128)(int64_t)hh[reg] * ((i128)1 << 32) +
                       (i128)((int64_t)hl[reg] + (int64_t)lh[reg]) * ((i128)1 << 16) + (i128)(int64_t)ll[reg];
        out[(q + 4 * reg) * 16 + r] = bt_wide{wide_lo(v), wide_hi(v)};   // row q + 4 reg of the tile, column r
    }
}

constexpr int kFoldBlock = 256;

// Blocks [0, gram_blocks): one thread per element of gram. Blocks past them (staged D only): the
// sum of one row of D.
__global__ __launch_bounds__(kFoldBlock) void gram_fold_kernel(const GramWork w, const int32_t gram_blocks) {
    const int tid = (int)threadIdx.x;
    if ((int32_t)blockIdx.x >= gram_blocks) {
        __shared__ int64_t s_part[kFoldBlock / 64];
        const int32_t i = (int32_t)blockIdx.x - gram_blocks;
        const int32_t* __restrict__ row = w.D + (int64_t)i * w.pitch;
        int64_t s = 0;
        for (int64_t t = tid; t < w.T; t += kFoldBlock) s += row[t];
        s = wave_sum_i64(s);
        if ((tid & 63) == 0) s_part[tid >> 6] = s;
        __syncthreads();
        if (tid == 0) {
            for (int k = 1; k < kFoldBlock / 64; ++k) s += s_part[k];
            w.sums[i] = s;
        }
        return;
    }
    const int64_t at = (int64_t)blockIdx.x * kFoldBlock + tid;
    if (at >= (int64_t)w.n * w.n) return;
    const int32_t i = (int32_t)(at / w.n), j = (int32_t)(at % w.n);
    const int32_t a = i <= j ? i : j, b = i <= j ? j : i;   // the element of the upper triangle
    const int32_t I = a >> 4, J = b >> 4;
    const int64_t tile = (int64_t)I * w.nt - (int64_t)I * (I - 1) / 2 + (J - I);
    const bt_wide* __restrict__ p = w.partial + tile * 256 + (a & 15) * 16 + (b & 15);
    i128 v = 0;
    for (int32_t c = 0; c < w.chunks; ++c) {
        const bt_wide x = p[(int64_t)c * w.tiles * 256];
        v += wide_join(x.lo, x.hi);
    }
    w.gram[at] = bt_wide{wide_lo(v), wide_hi(v)};
}

hipError_t launch_gram_walk(const LaneRef* lanes, const int32_t* high, const int32_t* low,
                            const int32_t* close, const Grid& g, const GramWork& w, int32_t from, int32_t to,
                            hipStream_t st) {
    if (w.n <= 0) return hipSuccess;
    launch_by_strategy(g.strategy, [&](auto strat) {
        hipLaunchKernelGGL(gram_walk_kernel<decltype(strat)::value>, dim3((unsigned)w.n), dim3(kTile), 0, st, lanes,
                           high, low, close, g, w, from, to);
    });
    return hipGetLastError();
}

hipError_t launch_gram(const GramWork& w, const GramPlan& pl, bool staged, hipStream_t st) {
    static_assert(kFoldBlock == 256, "plan.cpp plan_gram sets fold_block");
    if (w.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(gram_mfma_kernel, dim3((unsigned)pl.tiles, (unsigned)pl.chunks), dim3(64), 0, st, w);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    const int64_t cells = (int64_t)w.n * w.n;
    const int32_t gram_blocks = (int32_t)((cells + pl.fold_block - 1) / pl.fold_block);
    hipLaunchKernelGGL(gram_fold_kernel, dim3((unsigned)(gram_blocks + (staged ? w.n : 0))), dim3((unsigned)pl.fold_block),
                       0, st, w, gram_blocks);
    return hipGetLastError();
}

}  // namespace bt
