// k_ema.hip — EMA + rolling-OLS backtest (config 3) in the same tile pipeline as the SMA kernel:
// one workgroup per symbol, one lane per parameter.
//
// Hot path of BASELINE.json north_star (config 3), replacing the sleep in process_incoming_job
// (/root/reference/src/worker/process.rs:21-25). Spec: docs/oracle_spec.md §3-§5; checked
// bit-for-bit against oracle/oracle.c (orc_ema_ols).
//
// Every signal condition factors into per-indicator conditions, so a whole 64-bar tile of them
// is a handful of 64-bit words shared by all lanes:
//   (n, w): enter long  = [c*1e4 < e_n*(1e4-b)] & [N_w >= 0]
//           enter short = [c*1e4 > e_n*(1e4+b)] & [N_w <= 0] (and not long)
//           exit long = [c >= e_n], exit short = [c <= e_n]
// (the EMA as one sequential fp64 chain per span, lane = span, then ballots with lane = bar; the
// OLS numerator from the prefix rings in exact (wrapping) integer arithmetic). Each lane ANDs its
// words and walks only its position changes, O(1) accounting per change (tile_common.h). The
// Bollinger kernel of the same pipeline is k_boll.hip.
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "launch_run.h"
#include "lds_layout.h"
#include "plan.h"
#include "tile_common.h"

namespace bt {

namespace {

// wave priorities (s_setprio) of the pacing roles; BT_PRIO overrides them in the profiling build
// (scripts/gpu_prio_sweep.sh). The EMA chain at the top priority since it alone sets the 128-bar
// stage (round 6: helper A's tables moved to tasks and the chain wave out of the task rounds):
// config 3 2.565 -> 2.483 ms at 500 symbols, 1.598 -> 1.511 at 250 (at the
// base priority before, -0.5 to -1 %)
#ifndef BT_EMA_CHAIN_PRIO
#define BT_EMA_CHAIN_PRIO 3
#endif
#ifndef BT_EMA_WALK_PRIO
#define BT_EMA_WALK_PRIO 2
#endif
constexpr int kEmaChainPrio = BT_EMA_CHAIN_PRIO, kEmaWalkPrio = BT_EMA_WALK_PRIO;
// EMA+OLS walk accounts in int32 while the closes' total variation allows (unsplit runs)
#ifndef BT_EMA_NARROW
#define BT_EMA_NARROW 1
#endif
constexpr bool kEmaNarrow = BT_EMA_NARROW;

// Lane masks of 0 <= a and a <= 0 (int64) straight from the compare (tile_common.h vcmp_le_i32).
__device__ __forceinline__ uint64_t vcmp_ge0_i64(int64_t a) {
    uint64_t m;
    asm volatile("v_cmp_le_i64_e64 %0, 0, %1" : "=s"(m) : "v"(a));
    return m;
}
__device__ __forceinline__ uint64_t vcmp_le0_i64(int64_t a) {
    uint64_t m;
    asm volatile("v_cmp_ge_i64_e64 %0, 0, %1" : "=s"(m) : "v"(a));
    return m;
}

// State after every bar of a tile of a set/reset latch (set S and reset R disjoint), q = the
// state before bar 0: an add with carry, whose carry out of bit b is S_b | (~R_b & carry into b).
__device__ __forceinline__ uint64_t latch64(uint64_t S, uint64_t R, uint64_t q) {
    const uint64_t A = ~R;
    const uint64_t s1 = A + S;
    uint64_t cout = s1 < A;
    const uint64_t sum = s1 + q;
    cout |= sum < s1;
    return ((sum ^ A ^ S) >> 1) | (cout << 63);
}

}  // namespace

// Workgroup = parameter waves + helper A + helper B, one barrier per tile:
//   helper A, tile k+2: closes -> returns, drawdown sparse table, prefix rings;
//   helper B, tile k+2: the EMA chains (one sequential fp64 chain per span, lane = span);
//   every wave, tile k+1, after its own work: condition words, one task per span (4 ballots
//           over the EMA values) or per OLS window (exact numerator sign), grabbed from an LDS
//           counter;
//   parameter waves, tile k: the position after every bar from two coupled set/reset latches
//           over the condition words (latch64), then one trade per loop iteration over the
//           latches' edges, O(1) accounting per trade.
// SEG: bar segments as in boll_tile_kernel; besides the lanes' trade states a segment's start
// must agree on the EMA chains: a speculative segment starts each chain at its first scanned bar
// from an estimate of the true value (a truncated weighted sum of the closes before it, summed in
// parallel) and records the values entering its first accounted bar; fp64 chains from different
// starts meet bit for bit once the start's error has decayed below rounding (from the estimate:
// <= 4 spans of bars; from e = c: ~16), after which they are identical. The fix pass compares
// them too and re-walks from the true values.
template <bool PARITY, bool STAMPS, bool SEG, int TS>
__global__ __launch_bounds__(1024) void ema_tile_kernel(const SymDesc* __restrict__ syms,
                                                        const int32_t* __restrict__ close,
                                                        Grid g, Out out, int nextra, int lpw,
                                                        SegArgs sg, int fix_seg) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int nsp = g.na, nol = g.nb, R = g.ring;
    const TileLds LL = tile_lds_layout(0, R, nsp, nol, 0, TS);
    static_assert(TS == 1 || TS == 2, "64- or 128-bar stages");
    constexpr int CT = ema_ct_slots(TS), SL = ema_slots(TS), DS = ema_dst_slots(TS);
    // drawdown tables: built by the scan from its registers (64-bar stages, DSCAN), or as the
    // first tasks of the round that flags their stage (128-bar stages, DSTT: helper A then has
    // only the scans; config 3's task waves were idle ~2.5k cycles per tile while helper A paced
    // at ~3.9k with the tables)
    constexpr bool DSCAN = TS == 1, DSTT = TS == 2;
    uint64_t* r1 = reinterpret_cast<uint64_t*>(smem + LL.r1);  // sum_{i<x} c_i
    uint64_t* r2 = reinterpret_cast<uint64_t*>(smem + LL.r2);  // sum_{i<x} i*c_i (mod 2^64)
    int32_t* cts = reinterpret_cast<int32_t*>(smem + LL.ct);
    int64_t* qls = reinterpret_cast<int64_t*>(smem + LL.ql);
    Agg* dst = reinterpret_cast<Agg*>(smem + LL.dst);
    double* ebuf = reinterpret_cast<double*>(smem + LL.ebuf);  // [2][nsp][kEStride]
    uint64_t* words = reinterpret_cast<uint64_t*>(smem + LL.words);
    int32_t* win = reinterpret_cast<int32_t*>(smem + LL.win);
    int32_t* nars = reinterpret_cast<int32_t*>(smem + LL.nar);
    uint32_t* ctr = reinterpret_cast<uint32_t*>(smem + LL.ctr);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // waves: [0, npw) parameters, npw helper A, npw + 1 helper B, then `nextra` task-only waves
    const int nwaves = (int)(blockDim.x >> 6), npw = nwaves - 2 - nextra;
    const bool helperA = wave == npw, helperB = wave == npw + 1;
    const SymDesc sd = syms[blockIdx.x];
    const int B = sd.bars, ntiles = (B + kTile - 1) / kTile, P = g.n_params;
    // lpw parameter lanes per parameter wave (64, or fewer for shorter max-over-lanes walks)
    const int j = (blockIdx.y * npw + wave) * lpw + lane;
    const bool active = wave < npw && lane < lpw && j < P;
    const int pj = active ? j : 0;
    const int i_n = pj / nol, i_w = pj % nol;
    const int warm = max(g.a[i_n], g.b[i_w]) - 1;
    const int32_t* crow = close + sd.off;
    // tasks per stage: the drawdown tables of its tiles (DSTT), then one per span / OLS window
    const int nword = 4 * nsp + 2 * nol, ntask = max(nsp, nol) + (DSTT ? TS : 0);
    const int estage = nsp * kEStride;

    SegRange sr{0, 0, 0, 0, ntiles};
    double* ema_mine = nullptr;        // this (segment, symbol)'s chain record
    const double* ema_prev = nullptr;  // the previous segment's
    // this lane's record of segment sq, its address recomputed where it is used from an opaque
    // copy of the parameter index (a pointer kept live across the walk costs a VGPR pair, and the
    // split kernel runs at the 128-VGPR edge)
    auto seg_rec = [&](int sq) {
        int pje = pj;
        asm volatile("" : "+v"(pje));
        return sg.rec + (size_t)sq * gridDim.x * P + (size_t)blockIdx.x * P + pje;
    };
    if (SEG) {
        sr = seg_range(sg, fix_seg, ntiles, g.wmax);
        ema_mine = sg.ema + ((size_t)sr.seg * gridDim.x + blockIdx.x) * kEmaSegStride;
        if (sr.seg > 0) ema_prev = ema_mine - (size_t)gridDim.x * kEmaSegStride;
        if (fix_seg > 0) {  // re-walk if a lane's state or a span's chain value is not the true one
            const bool lane_differs = active && seg_start_differs(seg_rec(sr.seg), seg_rec(sr.seg - 1));
            const bool chain_differs = helperB && lane < nsp && ema_mine[lane] != ema_prev[64 + lane];
            if (!__syncthreads_or(lane_differs || chain_differs)) return;
            if (tid == 0) atomicAdd(sg.refixed, 1ULL);
        }
    }
    if (STAMPS) stamp_place(out.dbg, wave, lane);
    const int T_scan = sr.T_scan, T_walk = sr.T_walk, T_acct = sr.T_acct, T_end = sr.T_end;
    // the chains start at bar 0 with e = c there; a speculative segment's chains continue from
    // an estimate of the true values entering its first scanned bar, and the fix pass starts
    // them at its first bar from the true values
    const bool chain_injected = SEG && fix_seg > 0;
    const bool chain_est = SEG && fix_seg == 0 && T_scan > 0;
    const int chain_b0 = (chain_injected || chain_est) ? -1 : 0;
    const int chain_T0 = chain_injected ? T_acct : T_scan;

    // The estimate: e_ts = sum_{i<M} a (1-a)^i c_{ts-i} + (1-a)^M c_{ts-M+1}, the closed form of
    // the recurrence truncated after e^-36 of the weight (exact in real arithmetic when M reaches
    // bar 0). Every wave sums a strided share of the M bars, four spans at a time; the per-wave
    // sums go to ebuf (free until the first chain tile) and helper B adds them in wave order, so
    // the estimate is deterministic. Its rounding (~1e-14 relative) dies out in ~4 spans of
    // bars; the chains then meet the true ones bit for bit, and the fix pass catches any that
    // do not.
    int est_M = 0;
    if (chain_est) {
        const int ts = T_scan * kTile - 1;
        int maxspan = 1;
        for (int q = 0; q < nsp; ++q) maxspan = max(maxspan, g.a[q]);
        est_M = (int)min((int64_t)ts + 1, (int64_t)18 * ((int64_t)maxspan + 1) + 1);
        const int nchunk = (est_M + kTile - 1) / kTile;
        for (int q0 = 0; q0 < nsp; q0 += 4) {
            double acc[4], w[4], r[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int q = min(q0 + u, nsp - 1);
                const double a = 2.0 / ((double)g.a[q] + 1.0), lb = log2(1.0 - a);
                acc[u] = 0.0;
                w[u] = q0 + u < nsp ? a * exp2(lb * (double)(wave * kTile + lane)) : 0.0;
                r[u] = exp2(lb * (double)(kTile * nwaves));
            }
            for (int ch = wave; ch < nchunk; ch += 8 * nwaves) {
                int32_t cv[8];
#pragma unroll
                for (int v = 0; v < 8; ++v) {
                    const int i = (ch + v * nwaves) * kTile + lane;
                    cv[v] = i < est_M ? crow[ts - i] : 0;
                }
#pragma unroll
                for (int v = 0; v < 8; ++v) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        acc[u] = __builtin_fma(w[u], (double)cv[v], acc[u]);
                        w[u] *= r[u];
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                double s = acc[u];
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
                if (lane == 0 && q0 + u < nsp) ebuf[wave * nsp + q0 + u] = s;
            }
        }
    }

    for (int o = tid; o < nol; o += blockDim.x) win[o] = g.b[o];
    if (tid == 0) {
        // prefix entry x (sum over scanned bars < x) sits at x mod R: the scan's base is 0
        r1[(T_scan * kTile) % R] = 0;
        r2[(T_scan * kTile) % R] = 0;
        // task rounds are numbered by stage (flags), from 0
        *ctr = 0;
    }
    double alpha = 0.0, ema = 0.0;
    if (helperB && lane < nsp) {
        alpha = 2.0 / ((double)g.a[lane] + 1.0);
        if (chain_injected) ema = ema_prev[64 + lane];
    }
    const int winreg = lane < nol ? g.b[lane] : 1;  // OLS window lengths, lane = window
    const double lo_mult = (double)(10000 - g.band_bps), hi_mult = (double)(10000 + g.band_bps);
    __syncthreads();
    if (chain_est && helperB && lane < nsp) {
        double s = 0.0;
        for (int w2 = 0; w2 < nwaves; ++w2) s += ebuf[w2 * nsp + lane];
        const double tail = (double)crow[T_scan * kTile - est_M];
        ema = s + exp2(log2(1.0 - alpha) * (double)est_M) * tail;
    }

    TileCarry cy{0, (T_scan > 0 && T_scan * kTile - 1 < B) ? crow[T_scan * kTile - 1] : 0};
    uint64_t cy2 = 0;

    // Stages of TS tiles (TS = 2: 128 bars per barrier): stage st holds tiles T_scan + TS st ..
    // T_scan + TS st + TS - 1 (those past T_end absent). Per stage, one barrier:
    //   helper A: scans stage st + 2 (closes, returns, prefix rings; at TS = 1 the drawdown
    //             tables too);
    //   helper B: chains stage st + 2;
    //   the other waves: the tasks of stage st + 1 (DSTT: its tables, a stage after the scan,
    //             so they need two stages of buffers, not three: 80 KB per block at TS = 2; then
    //             one task per span / window over all its tiles);
    //   parameter waves: walk stage st, tile by tile.
    // Buffers by tile T: closes, returns, narrow flags T % CT (written st + 2, read st + 1 and st);
    // tables, chain values, words T % SL.
    const int nstage = (T_end - T_scan + TS - 1) / TS;
    auto scan = [&](int T, int32_t c) {
        const int s = T % CT, t0 = T * kTile, t = t0 + lane;
        int64_t inc2 = (int64_t)t * c;  // c = 0 past the end; scanned with the closes
        const int64_t pre = tile_scan<false, true>(c, B, t0, lane, cts + s * kTile, qls + s * 2 * kTile,
                                      dst + (T % DS) * kDstLevels * kTile, cy, DSCAN && !BT_ABL(g, 512),
                                      (SEG || !kEmaNarrow) ? nullptr : nars + s, 0, 0, &inc2);
        const int pt = ring_pos(T, lane, R);
        r1[pt] = (uint64_t)pre;
        r2[pt] = cy2 + (uint64_t)inc2;
        cy2 += (uint64_t)lane63_i64(inc2);
    };
    // drawdown sparse table of tile T from its staged closes (lane = bar; 0 past the end, as the
    // scan saw them)
    auto dbuild = [&](int T) {
        if (BT_ABL(g, 512)) return;  // (profiling ablation: no table)
        dst_build(cts[(T % CT) * kTile + lane], lane, dst + (T % DS) * kDstLevels * kTile);
    };

    // EMA chains of tile T, lane = span, from the tile's closes cl (lane = bar) that helper B
    // loads itself (no dependency on helper A's scan of the same tile):
    // e_t = e_{t-1} + alpha (c_t - e_{t-1}), three roundings, e_0 = c_0
    auto chain = [&](int T, int32_t cl) {
        if (SEG && T < chain_T0) return;  // fix pass: bars before the segment are not needed
        const int t1 = T * kTile;
        double* E = ebuf + (T % SL) * estage + lane * kEStride;
        // three dependent fp64 operations per bar; raising its priority over the walk no longer
        // pays (the walk, tasks, scan and chain all set the tile together: DESIGN.md §4.2)
        if (!BT_ABL(g, 32)) set_prio(BT_PRIO(g, 16, kEmaChainPrio));
        // the tile's closes as doubles, staged in span 0's row (lane = bar): each bar's close is
        // then one broadcast LDS read issued ahead of the chain instead of a readlane and a
        // conversion on it; span 0 overwrites bar b only after every span has read it (one
        // wave, LDS in program order)
        const double* CD = ebuf + (T % SL) * estage;
        if (nsp > 0) ebuf[(T % SL) * estage + lane] = (double)cl;
        if (lane < nsp && !BT_ABL(g, 256)) {  // profiling: 256 drops the chain, 128 its math
            if (BT_ABL(g, 128)) {
#pragma unroll
                for (int b = 0; b < kTile; ++b) E[b] = (double)__builtin_amdgcn_readlane(cl, b);
            } else if ((chain_b0 < t1 || chain_b0 >= t1 + kTile) && t1 + kTile <= B) {
                // 8 bars' closes read one chunk ahead (the reads precede, in program order, the
                // chain's stores that may alias them; opaque LDS pointers with immediate offsets
                // measured 6 % slower: DESIGN.md Appendix A)
                double* Ev = E;
                const double* Cv = CD;
                double nx[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) nx[u] = Cv[u];
#pragma unroll
                for (int c = 0; c < kTile / 8; ++c) {
                    double cur[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) cur[u] = nx[u];
                    if (c + 1 < kTile / 8) {
#pragma unroll
                        for (int u = 0; u < 8; ++u) nx[u] = Cv[8 * (c + 1) + u];
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        ema = ema + alpha * (cur[u] - ema);
                        Ev[8 * c + u] = ema;
                    }
                }
            } else {
#pragma unroll 1
                for (int b = 0; b < kTile; ++b) {
                    const double cd = (double)__builtin_amdgcn_readlane(cl, b);
                    if (t1 + b < B) ema = (t1 + b == chain_b0) ? cd : ema + alpha * (cd - ema);
                    E[b] = ema;
                }
            }
            // the values entering the first accounted bar, stored when the chain reaches them (a
            // register kept across the walk for them costs two VGPRs at the split kernel's edge);
            // a fix pass leaves the start record alone (other blockIdx.y blocks of the symbol
            // compare it with the previous segment's end, chain_differs, and may not have yet)
            if (SEG && fix_seg == 0 && T + 1 == T_acct) ema_mine[lane] = ema;
        }
        __builtin_amdgcn_s_setprio(0);
    };

    // with task-only waves present the parameter waves only walk: the walk is the per-tile
    // critical path (config 3: ~3.7k of ~4.9k cycles per tile on the parameter wave)
    const bool walk_only = nextra >= 2;
    // ... and helper B (the chain, which sets the stage with task waves idle) takes none either:
    // its grab after the chain would only find the round empty
    const bool chain_only = walk_only;
    const bool no_tasks = (walk_only && wave < npw) || (chain_only && helperB);
    const int ngrab = nwaves - (walk_only ? npw : 0) - (chain_only ? 1 : 0);

    // condition words of stage st (its TS tiles), tasks grabbed dynamically (round st), lane =
    // bar. Task o pairs span o with OLS window o (either may be absent) over every tile of the
    // stage: all LDS reads of the task are issued together, and the window length comes from a
    // register (winreg, lane = window), so a task costs one dependent LDS round trip after its
    // grab. A stage's tiles past T_end are computed on stale rows and not stored.
    auto flags = [&](int st) {
        if (no_tasks) return;
        const int T0 = T_scan + TS * st;
        const int nt = min(TS, T_end - T0);  // tiles of the stage (wave-uniform)
        double cd[TS], lhs[TS];
        uint64_t* Wd[TS];
        const double* Er[TS];
        int pt[TS];
        uint64_t P1[TS], P2[TS], tin[TS];
#pragma unroll
        for (int u = 0; u < TS; ++u) {
            const int T = T0 + u, t = T * kTile + lane;
            cd[u] = (double)cts[(T % CT) * kTile + lane];
            lhs[u] = cd[u] * 10000.0;
            Wd[u] = words + (T % SL) * nword;
            Er[u] = ebuf + (T % SL) * estage;
            pt[u] = ring_pos(T, lane, R);
            P1[u] = r1[pt[u]];
            P2[u] = r2[pt[u]];
            tin[u] = ballot(t < B);  // bars of the tile inside the series
        }
        const uint32_t base = (uint32_t)st * (uint32_t)(ntask + ngrab);
        uint32_t o = grab_value(grab_issue(ctr, lane)) - base;
        if (DSTT) {  // the round's first TS tasks: the tiles' drawdown tables
#pragma unroll 1
            while (o < (uint32_t)TS) {
                const uint32_t vn = grab_issue(ctr, lane);
                if ((int)o < nt) dbuild(T0 + (int)o);
                o = grab_value(vn) - base;
            }
            o -= TS;
        }
#pragma unroll 1
        while (o < (uint32_t)(ntask - (DSTT ? TS : 0))) {
            const uint32_t vn = grab_issue(ctr, lane);  // next task, read at the end
            const bool hs = (int)o < nsp, ho = (int)o < nol;  // wave-uniform
            const int Wn = nol <= 64 ? __builtin_amdgcn_readlane(winreg, (int)o & 63) : win[o];
            // unconditional reads at clamped / valid addresses (a task without a span or a window
            // leaves them unused): no select on the task's kind, which the compiler builds as a
            // VGPR bool
            const int erow = min((int)o, nsp - 1) * kEStride + lane;
            double e[TS];
            uint64_t r1j[TS], r2j[TS];
#pragma unroll
            for (int u = 0; u < TS; ++u) {
                const int pj = ring_back(pt[u], Wn, R);
                e[u] = Er[u][erow];
                r1j[u] = r1[pj];
                r2j[u] = r2[pj];
            }
            if (hs) {  // span: entry / exit conditions against the EMA
#pragma unroll
                for (int u = 0; u < TS; ++u) {
                    const uint64_t wa = __ballot(lhs[u] < e[u] * lo_mult), wb = __ballot(lhs[u] > e[u] * hi_mult);
                    const uint64_t wx = __ballot(cd[u] >= e[u]), wy = __ballot(cd[u] <= e[u]);
                    if (lane == 0 && u < nt) {
                        Wd[u][4 * o + 0] = wa;
                        Wd[u][4 * o + 1] = wb;
                        Wd[u][4 * o + 2] = wx;
                        Wd[u][4 * o + 3] = wy;
                    }
                }
            }
            if (ho) {  // OLS window: N = 2 T - (w-1) S over [t-w+1, t], exact modulo 2^64
                // 2 (sum i c_i - jj S) - (w - 1) S with one multiply, jj = t + 1 - w; masks
                // straight from the compares (a ballot of `valid && N >= 0` is a VGPR bool
                // compared again)
#pragma unroll
                for (int u = 0; u < TS; ++u) {
                    const int t = (T0 + u) * kTile + lane;
                    const uint64_t S = P1[u] - r1j[u];
                    const int64_t N = (int64_t)(2 * (P2[u] - r2j[u]) - (uint64_t)(int64_t)(2 * (t + 1 - Wn) + Wn - 1) * S);
                    const uint64_t vm = vcmp_le_i32(Wn, t + 1) & tin[u];  // jj >= 0 && t < B
                    const uint64_t wp = vcmp_ge0_i64(N) & vm, wn = vcmp_le0_i64(N) & vm;
                    if (lane == 0 && u < nt) {
                        Wd[u][4 * nsp + 2 * o] = wp;
                        Wd[u][4 * nsp + 2 * o + 1] = wn;
                    }
                }
            }
            o = grab_value(vn) - base - (DSTT ? TS : 0);
        }
    };

    // prologue: scan + chain stages 0 and 1; tables and words of stage 0
    int32_t cpre[TS];  // closes of the helpers' next stage, loaded a stage ahead
    if (helperA || helperB) {
        const int b0 = T_scan * kTile;
        int32_t c0[2 * TS];
#pragma unroll
        for (int u = 0; u < 2 * TS; ++u) c0[u] = ldc(crow, B, b0 + u * kTile + lane, 0);
#pragma unroll
        for (int u = 0; u < TS; ++u) cpre[u] = ldc(crow, B, b0 + (2 * TS + u) * kTile + lane, 0);
#pragma unroll
        for (int u = 0; u < 2 * TS; ++u) {
            if (T_scan + u < T_end) {
                if (helperA) scan(T_scan + u, c0[u]); else chain(T_scan + u, c0[u]);
            }
        }
    }
    __syncthreads();
    if (nstage > 0) flags(0);
    __syncthreads();

    TradeAcct a;
    acct_init(a);
    if (SEG && fix_seg > 0 && active) seg_inject(a, seg_rec(sr.seg - 1));
    const size_t gi = (size_t)blockIdx.x * P + pj;
    bt_trade* tr = (PARITY && active) ? out.trades + gi * out.trade_cap : nullptr;
    const int cap = out.trade_cap;

    StampAcc sa;
    // the walk of tile k (parameter waves)
    auto walk = [&](int k) {
        const int t0 = k * kTile;
        if (SEG && k == T_acct && active) {
            // first accounted tile: the state the (speculative) walk reached goes to the record
            // now; the burn-in's sums are dropped
            seg_write_start(seg_rec(sr.seg), a.pos, a.e);
            seg_reset_sums(a);
        }
        if (active && k >= T_walk && !BT_ABL(g, 8)) {
            set_prio(BT_PRIO(g, 18, kEmaWalkPrio));  // the walk is the per-tile critical path
            const int s = k % CT;
            const int32_t* cT = cts + s * kTile;
            const int64_t* ql = qls + s * 2 * kTile;
            const Agg* D = dst + (k % DS) * kDstLevels * kTile;
            const uint64_t* W = words + (k % SL) * nword;
            const uint64_t vm = bar_range_mask(t0, warm, B - 2);
            const uint64_t Aw = W[4 * i_n] & W[4 * nsp + 2 * i_w] & vm;
            const uint64_t Bw = W[4 * i_n + 1] & W[4 * nsp + 2 * i_w + 1] & vm & ~Aw;
            const uint64_t Xw = W[4 * i_n + 2] & vm, Yw = W[4 * i_n + 3] & vm;
            const int bl = B - 1 - t0;
            const uint64_t fb = bl < kTile ? (1ULL << bl) : 0ULL;  // forced exit (bl >= 0)
            // positions after every bar at once (replaces a per-trade search for the next entry
            // and exit bar): a long latch (set A, reset X or the forced exit) and a short one (set
            // B, reset Y); A and X are disjoint, B and Y too (band >= 0 and e > 0, so a close under
            // the lower band is under the EMA, fp64 rounding being monotone).
            // They are coupled only through "an entry needs a flat position": an entry bit
            // survives if the other side was not held before that bar. Bit b of the coupled masks
            // depends only on bits < b, so iterating to the fixpoint settles one more bar per pass
            // at least (one or two passes in practice).
            {
                const uint64_t RL = Xw | fb, RS = Yw | fb;
                const uint64_t lin = a.pos > 0, sin = a.pos < 0;
                uint64_t Ap = Aw, Bp = Bw, Lw, Sw;
#pragma unroll 1
                for (;;) {
                    Lw = latch64(Ap, RL, lin);
                    Sw = latch64(Bp, RS, sin);
                    const uint64_t An = Aw & ~((Sw << 1) | sin), Bn = Bw & ~((Lw << 1) | lin);
                    if (An == Ap && Bn == Bp) break;
                    Ap = An;
                    Bp = Bn;
                }
                const uint64_t Lb = (Lw << 1) | lin, Sb = (Sw << 1) | sin;
                const uint64_t EL = Lw & ~Lb;
                const uint64_t Ev0 = EL | (Sw & ~Sb), Xv0 = (Lb & ~Lw) | (Sb & ~Sw);
                // the trades of the tile; NARROW: gap and mdd in int32 while the closes' total
                // variation allows (tile_common.h Acct32; fills are at closes), one copy of the
                // loop per width, chosen per tile (wave-uniform)
                auto trades = [&](auto narrow_tag) {
                    constexpr bool NARROW = decltype(narrow_tag)::value;
                    Acct32 n32{(int32_t)a.gap, (int32_t)a.mdd};  // <= TV < 2^30 if NARROW
                    uint64_t Ev = Ev0, Xv = Xv0;
                    if (a.pos != 0 && Xv) {  // the position carried in closes first
                        const int x = __builtin_ctzll(Xv);
                        Xv &= Xv - 1;
                        const int32_t cx = cT[x];
                        const uint64_t qx = (uint64_t)ql[x], q2x = (uint64_t)ql[kTile + x];
                        const bool lg = a.pos > 0;
                        acct_close<PARITY, SEG, NARROW>(a, n32, t0 + x, cx,
                                                        agg_merge(a.agg, dst_query_w(D, a.sb, x)), tr, cap);
                        a.ps1 += lg ? qx : (uint64_t)0 - qx;
                        a.ps2 += q2x;
                        a.pos = 0;
                    }
#pragma unroll 1
                    while (Ev) {
                        if (STAMPS) sa.count(3);
                        // entry and exit bars are both known: every LDS read of the trade is
                        // issued together (an entry left open reads the tile's last bar, unused)
                        const int b = __builtin_ctzll(Ev);
                        Ev &= Ev - 1;
                        const bool hx = Xv != 0;
                        const int x = hx ? __builtin_ctzll(Xv) : kTile - 1;
                        Xv &= Xv - 1;
                        const int32_t cb = cT[b], cx = cT[x];
                        const uint64_t qb = (uint64_t)ql[b], q2b = (uint64_t)ql[kTile + b];
                        const uint64_t qx = (uint64_t)ql[x], q2x = (uint64_t)ql[kTile + x];
                        // whole 16-B entries, kept live: the side's drawdown or draw-up is then
                        // not re-read in a divergent branch (the compiler sank those reads once
                        // the accounting changed shape: config 3 +2 %)
                        const Agg st = dst_query_w(D, b, x);
                        const int np = ((EL >> b) & 1) ? 1 : -1;
                        a.ps1 += np > 0 ? (uint64_t)0 - qb : qb;
                        a.ps2 -= q2b;
                        acct_open(a, t0 + b, b, cb);
                        a.pos = np;
                        if (!hx) break;  // open at the tile end
                        acct_close<PARITY, SEG, NARROW>(a, n32, t0 + x, cx, st, tr, cap);
                        a.ps1 += np > 0 ? qx : (uint64_t)0 - qx;
                        a.ps2 += q2x;
                        a.pos = 0;
                    }
                    if (NARROW) {
                        a.gap = (uint32_t)n32.g;  // >= 0
                        a.mdd = (uint32_t)n32.m;
                    }
                };
                if (!SEG && kEmaNarrow && __builtin_amdgcn_readfirstlane(nars[s]))
                    trades(std::true_type{});
                else
                    trades(std::false_type{});
            }
            if (STAMPS) sa.mark(1);
            acct_tile_end(a, D, ql);
            __builtin_amdgcn_s_setprio(0);
        }
    };

    if (STAMPS) sa.begin();
    for (int st = 0; st < nstage; ++st) {
        const int k0 = T_scan + TS * st;
        if (helperA || helperB) {
#pragma unroll
            for (int u = 0; u < TS; ++u) {
                const int T = k0 + 2 * TS + u;
                if (T < T_end) {
                    if (helperA) scan(T, cpre[u]); else chain(T, cpre[u]);
                }
                cpre[u] = ldc(crow, B, (T + TS) * kTile + lane, 0);
            }
        }
        if (STAMPS) sa.mark(0);
#pragma unroll
        for (int u = 0; u < TS; ++u)
            if (k0 + u < T_end) walk(k0 + u);
        if (st + 1 < nstage && !BT_ABL(g, 2)) flags(st + 1);
        if (STAMPS) sa.mark(2);
        __syncthreads();
        if (STAMPS) sa.barrier();
    }
    if (STAMPS) sa.flush(out.dbg, wave < npw ? 0 : (helperA ? 1 : (helperB ? 2 : 3)), lane);
    if (SEG) {
        if (active) {
            // a segment with no bars never reached its first accounted tile: the state passes
            // through (flat, or the fix pass's injected one)
            if (T_acct >= T_end) seg_write_start(seg_rec(sr.seg), a.pos, a.e);
            seg_write_rest(a, seg_rec(sr.seg));
        }
        if (helperB && lane < nsp) {
            // a speculative segment whose chain never reached its first accounted bar records 0
            if (fix_seg == 0 && !(T_acct >= T_scan + 1 && T_acct <= T_end)) ema_mine[lane] = 0.0;
            ema_mine[64 + lane] = ema;  // after the segment's last bar
        }
        return;
    }
    if (active) acct_write(a, B, g.sqrt_ann, gi, out);
    wave_add_trades(out, active ? a.ntr : 0);
}

// The fold of a split run (tile_common.h seg_fold). Each tile kernel file has its own: a plain
// kernel is compiled ahead of the templates' instantiations, and the unsplit kernels' result write
// (sharpe_fx) keeps its instruction listing only with that conversion code compiled before them.
__global__ __launch_bounds__(256) void ema_seg_combine(const SymDesc* __restrict__ syms, int n_sym, int P,
                                                       const SegRec* __restrict__ rec, int G,
                                                       double sqrt_ann, Out out) {
    seg_fold(syms, n_sym, P, rec, G, sqrt_ann, out);
}

template <int TS>
static hipError_t launch_ema_ts(const SymDesc* syms, int32_t n_sym, const int32_t* close, const Grid& g,
                                const Out& out, bool parity, const SegArgs& seg, const LaunchPlan& pl,
                                hipStream_t st) {
    const dim3 block(pl.block);
    auto kernel = [&](auto v, dim3 grid, int s) {
        constexpr bool kPar = decltype(v)::value == Variant::kParity, kSeg = decltype(v)::value == Variant::kSeg;
#ifdef BT_PROFILING
        if (BT_ABL(g, 64) && s == 0) {  // the unsplit run or the speculative segments, stamped
            hipLaunchKernelGGL((ema_tile_kernel<false, true, kSeg, TS>), grid, block, pl.lds, st, syms, close, g, out, pl.xw, pl.lpw, seg, 0);
            return;
        }
#endif
        hipLaunchKernelGGL((ema_tile_kernel<kPar, false, kSeg, TS>), grid, block, pl.lds, st, syms, close, g, out, pl.xw, pl.lpw, seg, s);
    };
    auto fold = [&] { enqueue_fold(ema_seg_combine, seg.rec, syms, n_sym, g, pl.G, out, st); };
    return launch_run(kernel, fold, n_sym, parity, pl);
}

hipError_t launch_ema_ols(const SymDesc* syms, int32_t n_sym, const int32_t* close, const Grid& g,
                          const Out& out, bool parity, const SegArgs& seg, const LaunchPlan& pl,
                          hipStream_t st) {
    if (n_sym <= 0) return hipSuccess;
    return pl.ts == 2 ? launch_ema_ts<2>(syms, n_sym, close, g, out, parity, seg, pl, st)
                      : launch_ema_ts<1>(syms, n_sym, close, g, out, parity, seg, pl, st);
}

}  // namespace bt
