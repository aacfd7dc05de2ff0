// k_ddboot.hip — the drawdown bootstrap on the device (bt_drawdown_boot / bt_drawdown_boot_of,
// include/bt.h; semantics: docs/drawdown_spec.md). The start table is the reality check's
// (launch_boot_starts, k_boot.hip), so that the two calls draw the same bars.
//
// dd_kernel<STRAT, LDS>: one workgroup per lane. Its first wave walks the lane with a LaneWalk
// (walk_tile.h) and writes the exclusive prefix row Q[0..T] of the window's increments, as
// boot_kernel does, and takes the observed drawdown on the way: a wave prefix maximum of the tile's
// Q values under a carried peak, and per lane the largest peak - Q. dd_of_kernel<LDS>: the same for
// a staged row of increments. The row (Q, then one or two block tables) lives in dynamic LDS behind
// the workgroup's scratch (LDS) or in the lane's row of the arena.
//
// dd_table: a run of bars has the summary (s, h, l, dd): its sum, its largest and smallest prefix
// sum (the empty prefix included: h >= 0 >= l) and its largest drawdown from its own running peak.
// Summaries compose associatively (dd_mul); (0, 0, 0, 0) is the identity. W[s], s in [0, T), is the
// summary of the circular block of `len` bars that starts at bar s; s comes from Q, so an entry
// holds (h, l, dd). The doubled row is cut into chunks of len bars: a block that starts inside
// chunk c is the suffix of chunk c from s times the prefix of chunk c + 1 of the same length. The
// first sweep leaves the suffixes in W, the second composes the prefixes into them: O(T) whatever
// len. With many chunks a thread takes a chunk and walks it; with few a wave takes a chunk and scans
// it tile by tile with the operator (dd_wave_scan, plan.h, decides).
//
// dd_resample: thread = resample b; one step per block over the shared start table, the carry
// (X, peak, mdd) updated with the block's summary; only the cross term peak - X - l sees a
// drawdown whose peak and trough lie in different blocks. n_ge, the extremes, m1, m2 and the reach
// counts are wave sums of 32-bit limbs and one pass over the waves' partials. Integer maxima and
// sums: the bits do not depend on scheduling or on the row's home.
//
// dd_select: with Q > 0 the lane's B values stay with the workgroup (LDS, the lane's row of raw, or
// an arena row) and a most-significant-digit radix select of eight bits a pass finds every level at
// once, as k_tail.hip does, over the non-negative keys; passes above the top set bit of max_star
// are skipped.
#include <algorithm>

#include "plan.h"
#include "walk_tile.h"

namespace bt {

namespace {

constexpr int kDdThreads = 64 * kDdWaves;
constexpr int kDdQ = BT_DD_LEVELS_MAX, kDdR = BT_DD_LIMITS_MAX;
constexpr int kDdRedWords = 11 + kDdR;   // m1 and m2 in four 32-bit limbs each, n_ge, min, max, the reach counts

struct DdShared {
    uint64_t prefix[kDdQ];           // per level: the key's digits so far
    uint32_t rem[kDdQ];              // ... and the rank inside them (1-based)
    int64_t mdd_obs, max_star;
    uint64_t red[kDdWaves][kDdRedWords];
};
static_assert(kTailHistBytes + sizeof(DdShared) <= kDdFixedBytes, "the scratch fits in front of the row");
static_assert(kDdFixedBytes % 16 == 0, "the row is aligned");

struct DdSum {
    int64_t s, h, l, dd;
};
struct DdW {                         // a table entry: the block's sum comes from Q
    int64_t h, l, dd;
};
static_assert(sizeof(DdW) == kDdEntryBytes, "plan_ddboot sizes the tables");

__device__ __forceinline__ int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }
__device__ __forceinline__ int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }

__device__ __forceinline__ DdSum dd_one(int64_t x) { return DdSum{x, x > 0 ? x : 0, x < 0 ? x : 0, x < 0 ? -x : 0}; }
__device__ __forceinline__ DdSum dd_id() { return DdSum{0, 0, 0, 0}; }
// A then B
__device__ __forceinline__ DdSum dd_mul(const DdSum& A, const DdSum& B) {
    return DdSum{A.s + B.s, max64(A.h, A.s + B.h), min64(A.l, A.s + B.l), max64(max64(A.dd, B.dd), A.h - A.s - B.l)};
}
__device__ __forceinline__ DdSum dd_shfl_up(const DdSum& v, int d) {
    return DdSum{(int64_t)__shfl_up((long long)v.s, d, 64), (int64_t)__shfl_up((long long)v.h, d, 64),
                 (int64_t)__shfl_up((long long)v.l, d, 64), (int64_t)__shfl_up((long long)v.dd, d, 64)};
}
__device__ __forceinline__ DdSum dd_lane63(const DdSum& v) {
    return DdSum{lane63_i64(v.s), lane63_i64(v.h), lane63_i64(v.l), lane63_i64(v.dd)};
}

// The prefix sums of the doubled row: p in [0, 2T].
__device__ __forceinline__ int64_t dd_q2(const int64_t* q, int32_t T, int32_t p) { return p <= T ? q[p] : q[T] + q[p - T]; }

// W[s] for every s in [0, T) and blocks of `len` bars, 1 <= len <= T, by the whole workgroup. Ends
// with a barrier.
__device__ __forceinline__ void dd_table(const int64_t* q, DdW* W, const int32_t T, const int32_t len) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t nc = (T + len - 1) / len;          // chunks that hold a start
    if (!dd_wave_scan(T, len, kDdThreads)) {
        for (int32_t c = tid; c < nc; c += kDdThreads) {   // suffixes of chunk c, from its last bar down
            const int32_t lo = c * len;
            DdSum acc = dd_id();
            int64_t above = dd_q2(q, T, lo + len);
            for (int32_t p = lo + len - 1; p >= lo; --p) {
                const int64_t at = dd_q2(q, T, p);
                acc = dd_mul(dd_one(above - at), acc);
                above = at;
                if (p < T) W[p] = DdW{acc.h, acc.l, acc.dd};
            }
        }
        __syncthreads();
        for (int32_t c = tid; c < nc; c += kDdThreads) {   // prefixes of chunk c + 1 onto the suffixes of chunk c
            const int32_t lo = c * len, base = lo + len;
            const int64_t q_base = dd_q2(q, T, base);
            DdSum acc = dd_id();
            int64_t below = q_base;
            for (int32_t o = 1; o < len && lo + o < T; ++o) {
                const int64_t at = dd_q2(q, T, base + o);  // base + o <= lo + o + len - 1 + 1 <= 2T
                acc = dd_mul(acc, dd_one(at - below));
                below = at;
                const int32_t s = lo + o;
                const DdW w = W[s];
                const DdSum r = dd_mul(DdSum{q_base - q[s], w.h, w.l, w.dd}, acc);
                W[s] = DdW{r.h, r.l, r.dd};
            }
        }
        __syncthreads();
        return;
    }
    for (int32_t c = wave; c < nc; c += kDdWaves) {        // c is wave-uniform
        const int32_t lo = c * len;
        DdSum carry = dd_id();
        for (int32_t top = lo + len - 1; top >= lo; top -= 64) {   // lane 0 takes the highest bar of the tile
            const int32_t p = top - lane;
            DdSum v = p >= lo ? dd_one(dd_q2(q, T, p + 1) - dd_q2(q, T, p)) : dd_id();
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const DdSum y = dd_shfl_up(v, d);          // the bars above this lane's
                if (lane >= d) v = dd_mul(v, y);
            }
            v = dd_mul(v, carry);
            if (p >= lo && p < T) W[p] = DdW{v.h, v.l, v.dd};
            carry = dd_lane63(v);
        }
    }
    __syncthreads();
    for (int32_t c = wave; c < nc; c += kDdWaves) {
        const int32_t lo = c * len, base = lo + len;
        const int64_t q_base = dd_q2(q, T, base);
        DdSum carry = dd_id();
        for (int32_t o0 = 1; o0 < len && lo + o0 < T; o0 += 64) {
            const int32_t o = o0 + lane, s = lo + o;
            const bool on = o < len && s < T;
            DdSum v = on ? dd_one(dd_q2(q, T, base + o) - dd_q2(q, T, base + o - 1)) : dd_id();
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const DdSum y = dd_shfl_up(v, d);          // the bars below this lane's
                if (lane >= d) v = dd_mul(y, v);
            }
            v = dd_mul(carry, v);
            if (on) {
                const DdW w = W[s];
                const DdSum r = dd_mul(DdSum{q_base - q[s], w.h, w.l, w.dd}, v);
                W[s] = DdW{r.h, r.l, r.dd};
            }
            carry = dd_lane63(v);
        }
    }
    __syncthreads();
}

__device__ __forceinline__ int64_t wave_max_i64(int64_t x, int lane) { return lane63_i64(wave_maxscan_i64(x, lane)); }

// The observed drawdown, by the wave that builds Q: `peak` is the largest Q so far (wave-uniform),
// `mdd` each lane's largest peak - Q.
struct DdObs {
    int64_t peak = 0, mdd = 0;
    __device__ __forceinline__ void add(int64_t qv, bool valid, int lane) {
        const int64_t pm = max64(wave_maxscan_i64(valid ? qv : INT64_MIN, lane), peak);
        if (valid) mdd = max64(mdd, pm - qv);
        peak = lane63_i64(pm);
    }
};

// One block of a resample onto the carry.
__device__ __forceinline__ void dd_step(const int64_t* q, const DdW* W, int32_t T, int32_t s, int32_t len, int64_t& X,
                                        int64_t& peak, int64_t& mdd) {
    const int32_t e = s + len;
    const bool wrap = e > T;
    const int64_t sB = q[wrap ? T : e] - q[s] + (wrap ? q[e - T] : 0);
    const DdW w = W[s];
    mdd = max64(mdd, max64(w.dd, peak - X - w.l));
    peak = max64(peak, X + w.h);
    X += sB;
}

// The resampling of one lane from its row, by the whole workgroup; `vals`: where the B values stay
// for the selection (or nullptr), `raw`: the lane's row of raw_out (or nullptr).
__device__ __forceinline__ void dd_resample(const DdArgs& a, const int64_t* q, const DdW* W1, const DdW* W2, int64_t* vals,
                                            int64_t* raw, DdShared* sh) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t T = a.T, B = a.B, K = a.K;
    const int64_t obs = sh->mdd_obs;
    unsigned __int128 m1 = 0, m2 = 0;
    int64_t nge = 0, mn = INT64_MAX, mx = 0;
    int32_t reach[kDdR];
    int64_t lim[kDdR];
#pragma unroll
    for (int r = 0; r < kDdR; ++r) reach[r] = 0, lim[r] = r < a.R ? a.limits[r] : INT64_MAX;
    for (int32_t b = tid; b < B; b += kDdThreads) {
        const int32_t* __restrict__ sp = a.starts + b;
        int64_t X = 0, peak = 0, mdd = 0;
#pragma unroll 4
        for (int32_t j = 0; j < K - 1; ++j) dd_step(q, W1, T, sp[(int64_t)j * B], a.Lp, X, peak, mdd);
        dd_step(q, W2, T, sp[(int64_t)(K - 1) * B], a.last_len, X, peak, mdd);
        m1 += (unsigned __int128)(uint64_t)mdd;
        m2 += (unsigned __int128)(uint64_t)mdd * (uint64_t)mdd;
        nge += mdd >= obs ? 1 : 0;
        mn = min64(mn, mdd), mx = max64(mx, mdd);
#pragma unroll
        for (int r = 0; r < kDdR; ++r) reach[r] += mdd >= lim[r] ? 1 : 0;
        if (vals) vals[b] = mdd;
        if (raw) raw[b] = mdd;
    }
    uint64_t w[kDdRedWords];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        w[k] = (uint64_t)wave_sum_i64((int64_t)(uint64_t)(uint32_t)(m1 >> (32 * k)));
        w[4 + k] = (uint64_t)wave_sum_i64((int64_t)(uint64_t)(uint32_t)(m2 >> (32 * k)));
    }
    w[8] = (uint64_t)wave_sum_i64(nge);
    w[9] = (uint64_t)-wave_max_i64(-mn, lane);       // INT64_MAX where the thread had no resample: -mn does not overflow
    w[10] = (uint64_t)wave_max_i64(mx, lane);
#pragma unroll
    for (int r = 0; r < kDdR; ++r) w[11 + r] = (uint64_t)wave_sum_i64((int64_t)reach[r]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kDdRedWords; ++k) sh->red[wave][k] = w[k];
    }
    __syncthreads();                 // the partials, and every wave's vals
    if (tid == 0) {
        unsigned __int128 s1 = 0, s2 = 0;
        int64_t ng = 0, lo = INT64_MAX, hi = 0, rc[kDdR];
#pragma unroll
        for (int r = 0; r < kDdR; ++r) rc[r] = 0;
        for (int v = 0; v < kDdWaves; ++v) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                s1 += (unsigned __int128)sh->red[v][k] << (32 * k);
                s2 += (unsigned __int128)sh->red[v][4 + k] << (32 * k);
            }
            ng += (int64_t)sh->red[v][8];
            lo = min64(lo, (int64_t)sh->red[v][9]);
            hi = max64(hi, (int64_t)sh->red[v][10]);
#pragma unroll
            for (int r = 0; r < kDdR; ++r) rc[r] += (int64_t)sh->red[v][11 + r];
        }
        sh->max_star = hi;
        if (a.rec) {
            bt_dd_lane* __restrict__ o = a.rec + blockIdx.x;
            o->sum = q[T];
            o->mdd = obs;
            o->n_ge = ng;
            o->min_star = lo, o->max_star = hi;
            o->m1.lo = (uint64_t)s1, o->m1.hi = (int64_t)(uint64_t)(s1 >> 64);
            o->m2.lo = (uint64_t)s2, o->m2.hi = (int64_t)(uint64_t)(s2 >> 64);
        }
        if (a.reach)
            for (int r = 0; r < a.R; ++r) a.reach[(int64_t)blockIdx.x * a.R + r] = rc[r];
    }
    __syncthreads();                 // max_star
}

// The k_j-th smallest of vals[0 .. B) at every level, by the whole workgroup.
__device__ __forceinline__ void dd_select(const DdArgs& a, const int64_t* vals, DdShared* sh, uint32_t* hist) {
    if (!a.q || a.Q < 1) return;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t Q = a.Q, B = a.B;
    if (tid < Q) {
        sh->rem[tid] = (uint32_t)(((uint64_t)B * (uint64_t)a.levels[tid] + 999999ull) / 1000000ull);   // in [1, B]
        sh->prefix[tid] = 0;
    }
    const uint64_t top = (uint64_t)sh->max_star;
    const int bits = top ? 64 - __builtin_clzll(top) : 0;
    for (int shift = 8 * ((bits + 7) / 8 - 1); shift >= 0; shift -= 8) {   // shift <= 48: the keys are below 2^53
        for (int i = tid; i < Q * 256; i += kDdThreads) hist[i] = 0;
        __syncthreads();             // the histograms are clear, the levels' state of the pass before is written
        for (int32_t i0 = wave * 64; i0 < B; i0 += kDdThreads) {   // i0 is wave-uniform: whole waves enter
            const int32_t i = i0 + lane;
            const bool on = i < B;
            const uint64_t key = on ? (uint64_t)vals[i] : 0ull;
            const uint32_t bin = (uint32_t)(key >> shift) & 255u;
            for (int j = 0; j < Q; ++j) {
                const bool hit = on && ((key ^ sh->prefix[j]) >> (shift + 8)) == 0;   // the digits above agree
                const uint64_t hm = __ballot(hit);
                if (!hm) continue;
                const int first = __builtin_ctzll(hm);
                const uint32_t b0 = (uint32_t)lane_i32((int32_t)bin, first);
                if (__ballot(hit && bin == b0) == hm) {      // one bin: a row of equal values adds once a wave
                    if (lane == first) atomicAdd(&hist[j * 256 + b0], (uint32_t)__popcll(hm));
                } else if (hit) {
                    atomicAdd(&hist[j * 256 + bin], 1u);
                }
            }
        }
        __syncthreads();
        for (int j = wave; j < Q; j += kDdWaves) {   // a wave per level, four bins per lane
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
                sh->prefix[j] |= (uint64_t)(4 * lane + b) << shift;
                sh->rem[j] = rem - before;
            }
        }
        __syncthreads();
    }
    __syncthreads();                 // prefix and rem of a call without a pass
    if (tid < Q) a.q[(int64_t)blockIdx.x * Q + tid] = (int64_t)sh->prefix[tid];
}

// Everything after Q: the tables, the resampling, the selection.
template <bool LDS>
__device__ __forceinline__ void dd_finish(const DdArgs& a, unsigned char* smem, unsigned char* row) {
    uint32_t* hist = reinterpret_cast<uint32_t*>(smem);
    DdShared* sh = reinterpret_cast<DdShared*>(smem + kTailHistBytes);
    const int64_t* q = reinterpret_cast<const int64_t*>(row);
    DdW* W1 = reinterpret_cast<DdW*>(row + a.r_w1);
    DdW* W2 = reinterpret_cast<DdW*>(row + a.r_w2);
    // a call with one block per resample uses the last block's table alone
    if (a.K > 1) dd_table(q, W1, a.T, a.Lp);
    if (a.K == 1 || a.r_w2 != a.r_w1) dd_table(q, W2, a.T, a.last_len);
    int64_t* raw = a.raw ? a.raw + (int64_t)blockIdx.x * a.B : nullptr;
    int64_t* vals = nullptr;
    if (a.q && a.Q > 0)
        vals = a.l_vals ? reinterpret_cast<int64_t*>(smem + a.l_vals) : raw ? raw : a.vals + (int64_t)blockIdx.x * a.v_pitch;
    dd_resample(a, q, W1, W2, vals, vals == raw ? nullptr : raw, sh);
    dd_select(a, vals, sh, hist);
}

}  // namespace

// STRAT: bt_strategy; LDS: the row lives in dynamic LDS behind kDdFixedBytes, else in row blockIdx.x
// of a.rows. blockIdx.x = the lane of the chunk, lane0 + blockIdx.x that of the call.
template <int STRAT, bool LDS>
__global__ __launch_bounds__(kDdThreads) void dd_kernel(const DdArgs a, const int32_t* __restrict__ high,
                                                        const int32_t* __restrict__ low,
                                                        const int32_t* __restrict__ close, const Grid g) {
    extern __shared__ __align__(16) unsigned char dd_smem[];
    DdShared* sh = reinterpret_cast<DdShared*>(dd_smem + kTailHistBytes);
    unsigned char* row = LDS ? dd_smem + kDdFixedBytes : a.rows + (int64_t)blockIdx.x * a.pitch;
    int64_t* q = reinterpret_cast<int64_t*>(row);
    const int tid = (int)threadIdx.x;
    LaneRef L;
    if (a.lanes) {
        L = a.lanes[blockIdx.x];
    } else {
        const int64_t i = a.lane0 + blockIdx.x;
        const int32_t gi = (int32_t)(i / a.P);
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
        DdObs obs;
        if (tid == 0) q[0] = 0;
        for (int32_t t0 = 0; t0 < end; t0 += kTile) {
            const LaneTile o = lw.step(t0);
            if (t0 + kTile < a.from) continue;            // before the tile of bar from - 1
            const int32_t bl = a.from - 1 - t0;           // that bar's lane in this tile
            if (bl >= 0 && bl < kTile) base = lane_i64(o.E, bl);
            const int32_t t = t0 + tid;
            const bool in = t >= a.from && t < end;
            if (in) q[t - a.from + 1] = o.E - base;       // t - from + 1 <= filled <= T
            obs.add(o.E - base, in, tid);
        }
        const int64_t m = wave_max_i64(obs.mdd, tid);
        if (tid == 0) sh->mdd_obs = m;
    }
    __syncthreads();
    // q[filled + 1 .. T] = q[filled]: the bars past the row's end add nothing
    const int64_t tail = q[filled];
    for (int32_t k = filled + 1 + tid; k <= a.T; k += kDdThreads) q[k] = tail;
    __syncthreads();
    dd_finish<LDS>(a, dd_smem, row);
}

template <bool LDS>
__global__ __launch_bounds__(kDdThreads) void dd_of_kernel(const DdArgs a) {
    extern __shared__ __align__(16) unsigned char dd_smem[];
    DdShared* sh = reinterpret_cast<DdShared*>(dd_smem + kTailHistBytes);
    unsigned char* row = LDS ? dd_smem + kDdFixedBytes : a.rows + (int64_t)blockIdx.x * a.pitch;
    int64_t* q = reinterpret_cast<int64_t*>(row);
    const int tid = (int)threadIdx.x;
    const int32_t* __restrict__ drow = a.d + (int64_t)blockIdx.x * a.d_pitch;
    if (tid < kTile) {
        int64_t carry = 0;
        DdObs obs;
        if (tid == 0) q[0] = 0;
        for (int32_t k0 = 0; k0 < a.T; k0 += kTile) {
            const int32_t k = k0 + tid;
            const bool in = k < a.T;
            const int64_t s = carry + wave_iscan_i64(in ? (int64_t)drow[k] : 0);
            if (in) q[k + 1] = s;
            obs.add(s, in, tid);
            carry = lane63_i64(s);
        }
        const int64_t m = wave_max_i64(obs.mdd, tid);
        if (tid == 0) sh->mdd_obs = m;
    }
    __syncthreads();
    dd_finish<LDS>(a, dd_smem, row);
}

// Dynamic LDS above 64 KB has to be asked for, per kernel: once a call, before its chunks, for the one
// kernel the call launches. Both homes can pass 64 KB: the LDS home by the row, the arena home by
// the B values of the selection.
hipError_t prepare_dd(const DdPlan& pl, bool staged, const Grid& g) {
    static_assert(kDdLdsBytes <= kCuLdsBytes, "a workgroup's LDS is a CU's at most");
    if (pl.lds_bytes <= 64 * 1024) return hipSuccess;
    const void* kernel = nullptr;
    if (staged) {
        kernel = pl.row_mode == 1 ? reinterpret_cast<const void*>(dd_of_kernel<true>)
                                  : reinterpret_cast<const void*>(dd_of_kernel<false>);
    } else {
        launch_by_strategy(g.strategy, [&](auto strat) {
            constexpr int S = decltype(strat)::value;
            kernel = pl.row_mode == 1 ? reinterpret_cast<const void*>(dd_kernel<S, true>)
                                      : reinterpret_cast<const void*>(dd_kernel<S, false>);
        });
    }
    return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds_bytes);
}

hipError_t launch_dd_walk(const DdArgs& a, int32_t m, const DdPlan& pl, const int32_t* high, const int32_t* low,
                          const int32_t* close, const Grid& g, hipStream_t st) {
    if (m <= 0) return hipSuccess;
    launch_by_strategy(g.strategy, [&](auto strat) {
        constexpr int S = decltype(strat)::value;
        if (pl.row_mode == 1)
            hipLaunchKernelGGL((dd_kernel<S, true>), dim3((unsigned)m), dim3((unsigned)pl.block), pl.lds_bytes, st, a,
                               high, low, close, g);
        else
            hipLaunchKernelGGL((dd_kernel<S, false>), dim3((unsigned)m), dim3((unsigned)pl.block), pl.lds_bytes, st, a,
                               high, low, close, g);
    });
    return hipGetLastError();
}

hipError_t launch_dd_of(const DdArgs& a, int32_t m, const DdPlan& pl, hipStream_t st) {
    if (m <= 0) return hipSuccess;
    if (pl.row_mode == 1)
        hipLaunchKernelGGL(dd_of_kernel<true>, dim3((unsigned)m), dim3((unsigned)pl.block), pl.lds_bytes, st, a);
    else
        hipLaunchKernelGGL(dd_of_kernel<false>, dim3((unsigned)m), dim3((unsigned)pl.block), pl.lds_bytes, st, a);
    return hipGetLastError();
}

}  // namespace bt
