// k_surface.hip — reductions of a run's S x P summaries (bt_surface, docs/surface_spec.md): per
// parameter an aggregate over every symbol (bt_param_agg), per symbol its best lane (bt_topk_rec).
//
// One pass reads every 48-B record once. Lanes run along p, so a wave reads 64 consecutive
// records (3 KB) of a row; grid x tiles the parameters, grid y cuts the rows into chunks
// (plan.cpp plan_surface), and every lane walks its chunk's rows with its column's aggregate in
// registers. The same pass gives the per-symbol best: a wave holds 64 lanes of one row, so a
// cross-lane maximum of the order key and a ballot name the tile's winner (the lowest param among
// equal keys), whose lane writes the record.
//   surface_pass        -> partial[chunk][p] (bt_param_agg), best_partial[row][tile] (bt_topk_rec)
//   surface_fold_params -> agg[p]:  the chunks' partials merged (surface_spec §3), in two steps
//                          (chunks -> fold_ways -> 1) when there are many
//   surface_fold_best   -> best[s]: the tiles' winners merged, one wave per row
// Everything is order-independent (integer sums, int128 lo/hi pairs with carry, min/max with the
// id tie rule), so the folds need no fixed order, no atomics and no floating-point sum.
#include "internal.h"
#include "plan.h"

namespace bt {

namespace {

__device__ __forceinline__ double key_to_double(uint64_t k) {  // inverse of order_key
    const uint64_t u = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFULL) : ~k;
    return __longlong_as_double((long long)u);
}

// qs of surface_spec §1: clamp(sharpe, +-2^15) * 2^32 (exact), rounded half to even
__device__ __forceinline__ long long sharpe_fixed(double sh) {
    double x = sh == sh ? sh : 0.0;
    x = x < -32768.0 ? -32768.0 : (x > 32768.0 ? 32768.0 : x);
    return (long long)rint(x * 4294967296.0);
}

__device__ __forceinline__ void add128(uint64_t& lo, int64_t& hi, uint64_t blo, int64_t bhi) {
    const uint64_t nl = lo + blo;
    hi = (int64_t)((uint64_t)hi + (uint64_t)bhi + (nl < lo ? 1u : 0u));
    lo = nl;
}

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint64_t o = __shfl_xor((unsigned long long)v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ int wave_min_i32(int v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const int o = __shfl_xor(v, d, 64);
        v = o < v ? o : v;
    }
    return v;
}

// a += b, aggregates of disjoint symbol sets (surface_spec §3)
__device__ __forceinline__ void agg_merge(bt_param_agg& a, const bt_param_agg& b) {
    if (b.n_sym == 0) return;
    if (a.n_sym == 0) {
        a = b;
        return;
    }
    a.n_sym += b.n_sym;
    a.n_traded += b.n_traded;
    a.n_win += b.n_win;
    a.n_pos += b.n_pos;
    a.trades += b.trades;
    a.pnl += b.pnl;
    a.exposure += b.exposure;
    a.mdd_max = b.mdd_max > a.mdd_max ? b.mdd_max : a.mdd_max;
    const uint64_t amax = order_key(a.sharpe_max), bmax = order_key(b.sharpe_max);
    if (bmax > amax || (bmax == amax && b.sym_max < a.sym_max)) {
        a.sharpe_max = b.sharpe_max;
        a.sym_max = b.sym_max;
    }
    const uint64_t amin = order_key(a.sharpe_min), bmin = order_key(b.sharpe_min);
    if (bmin < amin || (bmin == amin && b.sym_min < a.sym_min)) {
        a.sharpe_min = b.sharpe_min;
        a.sym_min = b.sym_min;
    }
    add128(a.ss1_lo, a.ss1_hi, b.ss1_lo, b.ss1_hi);
    add128(a.ss2_lo, a.ss2_hi, b.ss2_lo, b.ss2_hi);
}

}  // namespace

// grid (p_blocks, chunks), block a multiple of 64. Lanes past P read the row's last record and
// contribute nothing; a wave wholly past P leaves at once.
template <bool AGG, bool BEST>
__global__ __launch_bounds__(256) void surface_pass(const bt_summary* __restrict__ sum,
                                                    const int32_t* __restrict__ ids, int32_t id_stride,
                                                    int32_t P, int32_t rows_per_chunk, int32_t rows_rem,
                                                    int32_t p_tiles, bt_param_agg* __restrict__ partial,
                                                    bt_topk_rec* __restrict__ best_partial) {
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const int tile = p >> 6;  // wave-uniform
    if (tile * 64 >= P) return;
    const bool valid = p < P;
    const int pc = valid ? p : P - 1;
    const int lane = (int)(threadIdx.x & 63);
    const int c = (int)blockIdx.y;
    const int r0 = c * rows_per_chunk + (c < rows_rem ? c : rows_rem);
    const int r1 = r0 + rows_per_chunk + (c < rows_rem ? 1 : 0);

    int32_t n_sym = 0, n_traded = 0, n_win = 0, n_pos = 0;
    int64_t trades = 0, pnl_sum = 0, expo = 0, mdd_max = INT64_MIN;
    uint64_t kmax = 0, kmin = 0;
    int32_t idmax = -1, idmin = -1;
    uint64_t s1lo = 0, s2lo = 0;
    int64_t s1hi = 0, s2hi = 0;

    // the next row's loads are issued before this row is reduced: two rows in flight per wave
    struct Row {
        uint4 a, b;
        uint2 d;
        int32_t id;
    };
    auto load_row = [&](int s) {
        const bt_summary* rec = sum + ((int64_t)s * P + pc);
        // 48 B: two 16-B loads and the Sharpe's 8 bytes (the hash is not read)
        return Row{*reinterpret_cast<const uint4*>(rec), *(reinterpret_cast<const uint4*>(rec) + 1),
                   *(reinterpret_cast<const uint2*>(rec) + 4), ids[(int64_t)s * id_stride]};
    };
    Row next{};
    if (r0 < r1) next = load_row(r0);
    for (int s = r0; s < r1; ++s) {
        const Row row = next;
        if (s + 1 < r1) next = load_row(s + 1);
        const uint4 a = row.a, b = row.b;
        const uint2 d = row.d;
        const int32_t id = row.id;
        const int32_t ntr = (int32_t)a.x, status = (int32_t)a.y;
        const int64_t pnl = (int64_t)(((uint64_t)a.w << 32) | a.z);
        const int64_t mdd = (int64_t)(((uint64_t)b.y << 32) | b.x);
        const int64_t ex = (int64_t)(((uint64_t)b.w << 32) | b.z);
        const uint64_t shbits = ((uint64_t)d.y << 32) | d.x;
        const double sh = __longlong_as_double((long long)shbits);
        const uint64_t key = order_key(sh);
        if (AGG) {
            const bool ok = valid && status == 0;
            const bool first = n_sym == 0;
            if (ok) {
                n_sym += 1;
                n_traded += ntr > 0 ? 1 : 0;
                n_win += pnl > 0 ? 1 : 0;
                n_pos += sh > 0.0 ? 1 : 0;
                trades += ntr;
                pnl_sum += pnl;
                expo += ex;
                mdd_max = mdd > mdd_max ? mdd : mdd_max;
                if (first || key > kmax || (key == kmax && id < idmax)) {
                    kmax = key;
                    idmax = id;
                }
                if (first || key < kmin || (key == kmin && id < idmin)) {
                    kmin = key;
                    idmin = id;
                }
                const long long q = sharpe_fixed(sh);
                add128(s1lo, s1hi, (uint64_t)q, (int64_t)(q >> 63));
                const uint64_t m = (uint64_t)(q < 0 ? -q : q);  // |q| <= 2^47
                add128(s2lo, s2hi, m * m, (int64_t)__umul64hi(m, m));
            }
        }
        if (BEST) {
            // every record's key is >= 0 and a lane past P offers 0 but never votes
            const uint64_t top = wave_max_u64(valid ? key : 0ULL);
            const unsigned long long votes = __ballot(valid && key == top);
            if (lane == __ffsll(votes) - 1)
                best_partial[(int64_t)s * p_tiles + tile] = bt_topk_rec{sh, id, p, pnl};
        }
    }
    if (AGG && valid) {
        bt_param_agg o;
        const bool any = n_sym > 0;
        o.n_sym = n_sym;
        o.n_traded = n_traded;
        o.n_win = n_win;
        o.n_pos = n_pos;
        o.trades = trades;
        o.pnl = pnl_sum;
        o.exposure = expo;
        o.mdd_max = any ? mdd_max : 0;
        o.sharpe_max = any ? key_to_double(kmax) : 0.0;
        o.sharpe_min = any ? key_to_double(kmin) : 0.0;
        o.sym_max = idmax;
        o.sym_min = idmin;
        o.ss1_lo = s1lo;
        o.ss1_hi = s1hi;
        o.ss2_lo = s2lo;
        o.ss2_hi = s2hi;
        partial[(int64_t)c * P + p] = o;
    }
}

// Partials merged, one lane per parameter: grid (64-lane tiles of P, n_out), one wave per block.
// Wave (tile, j) merges in[j], in[j + n_out], in[j + 2 n_out], ... (< n_in) and writes out[j]. With
// many chunks the launcher runs it twice (chunks -> fold_ways -> 1), so that no wave walks more
// than about sqrt(chunks) partials one after the other. Four loads are in flight at a time. A
// partial without counted rows is skipped by the merge, and an aggregate that stays empty is the
// canonical empty record the pass wrote.
__global__ __launch_bounds__(64) void surface_fold_params(const bt_param_agg* __restrict__ in, int32_t P,
                                                          int32_t n_in, bt_param_agg* __restrict__ out) {
    const int p = (int)(blockIdx.x * 64 + threadIdx.x);
    if (p >= P) return;
    const int j = (int)blockIdx.y, step = (int)gridDim.y;
    bt_param_agg a = in[(int64_t)j * P + p];
    for (int c = j + step; c < n_in; c += 4 * step) {
        bt_param_agg b0, b1, b2, b3;
        b0 = in[(int64_t)c * P + p];
        b1.n_sym = b2.n_sym = b3.n_sym = 0;
        if (c + step < n_in) b1 = in[(int64_t)(c + step) * P + p];
        if (c + 2 * step < n_in) b2 = in[(int64_t)(c + 2 * step) * P + p];
        if (c + 3 * step < n_in) b3 = in[(int64_t)(c + 3 * step) * P + p];
        agg_merge(a, b0);
        agg_merge(a, b1);
        agg_merge(a, b2);
        agg_merge(a, b3);
    }
    out[(int64_t)j * P + p] = a;
}

// One wave per row: the tiles' winners merged by (order key descending, param ascending).
__global__ __launch_bounds__(256) void surface_fold_best(const bt_topk_rec* __restrict__ best_partial,
                                                         int32_t S, int32_t p_tiles,
                                                         bt_topk_rec* __restrict__ best) {
    const int64_t row = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;  // wave-uniform
    if (row >= S) return;
    const int lane = (int)(threadIdx.x & 63);
    const bt_topk_rec* tiles = best_partial + row * p_tiles;
    bool have = false;
    bt_topk_rec mine{};
    uint64_t mk = 0;
    for (int t = lane; t < p_tiles; t += 64) {  // tiles ascend in param: a later one wins only on a greater key
        const bt_topk_rec r = tiles[t];
        const uint64_t k = order_key(r.sharpe);
        if (!have || k > mk) {
            mine = r;
            mk = k;
            have = true;
        }
    }
    const uint64_t top = wave_max_u64(have ? mk : 0ULL);
    const bool cand = have && mk == top;
    const int pmin = wave_min_i32(cand ? mine.param : INT32_MAX);
    const unsigned long long votes = __ballot(cand && mine.param == pmin);
    if (lane == __ffsll(votes) - 1) best[row] = mine;
}

hipError_t launch_surface(const bt_summary* sum, const int32_t* ids, int32_t id_stride, int32_t S,
                          int32_t P, const SurfacePlan& pl, const SurfaceWork& w, hipStream_t st) {
    const bool agg = w.agg != nullptr, best = w.best != nullptr && S > 0;
    if (!agg && !best) return hipSuccess;
    const dim3 grid((unsigned)pl.p_blocks, (unsigned)pl.chunks), block((unsigned)pl.block);
    if (agg && best)
        hipLaunchKernelGGL((surface_pass<true, true>), grid, block, 0, st, sum, ids, id_stride, P,
                           pl.rows_per_chunk, pl.rows_rem, pl.p_tiles, w.partial, w.best_partial);
    else if (agg)
        hipLaunchKernelGGL((surface_pass<true, false>), grid, block, 0, st, sum, ids, id_stride, P,
                           pl.rows_per_chunk, pl.rows_rem, pl.p_tiles, w.partial, w.best_partial);
    else
        hipLaunchKernelGGL((surface_pass<false, true>), grid, block, 0, st, sum, ids, id_stride, P,
                           pl.rows_per_chunk, pl.rows_rem, pl.p_tiles, w.partial, w.best_partial);
    if (agg) {
        const unsigned tiles = (unsigned)pl.p_tiles;
        const bt_param_agg* src = w.partial;
        int32_t n = pl.chunks;
        if (pl.fold_ways > 0) {
            hipLaunchKernelGGL(surface_fold_params, dim3(tiles, (unsigned)pl.fold_ways), dim3(64), 0, st, src, P, n,
                               w.fold);
            src = w.fold;
            n = pl.fold_ways;
        }
        hipLaunchKernelGGL(surface_fold_params, dim3(tiles, 1), dim3(64), 0, st, src, P, n, w.agg);
    }
    if (best)
        hipLaunchKernelGGL(surface_fold_best, dim3((unsigned)(((int64_t)S + 3) / 4)), dim3(256), 0, st,
                           (const bt_topk_rec*)w.best_partial, S, pl.p_tiles, w.best);
    return hipGetLastError();
}

}  // namespace bt
