// lds_layout.h — how the strategy kernels carve up their dynamic LDS, with the constants the
// layouts use. Included by the kernels (k_sma.hip, k_ema.hip, k_boll.hip), which take their buffers from
// these offsets, and by the host planner (plan.cpp), which checks and requests the same totals.
#pragma once
#include "device_common.h"

namespace bt {

// ---------------------------------------------------------------------------- SMA (k_sma.hip)
constexpr int kKS = kTile + 4;        // int32 key row stride: rows 16-B aligned for b128 reads
constexpr int kStages = 3;            // tile buffers in flight (cT, Q)
constexpr int kDstStages = 2;         // drawdown tables: built in interval k - 1, read in k
constexpr int kRingMirror = kTile;    // ring entries repeated past its end (ring_store)

struct SmaLds {                       // byte offsets into dynamic LDS
    size_t ring, keys, dst, ct, ql, nar, ctr, total;
};

__host__ __device__ inline SmaLds sma_lds_layout(int ring, int nw) {
    SmaLds L;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o += (bytes + 15) & ~size_t(15); return r; };
    L.ring = take((size_t)(ring + kRingMirror) * 8);
    const int nwp = (nw + kKeyGrab - 1) / kKeyGrab * kKeyGrab;  // key rows: whole groups
    L.keys = take((size_t)2 * nwp * kKS * 4);
    L.dst = take((size_t)kDstStages * kDstLevels * kTile * sizeof(Agg));
    L.ct = take((size_t)kStages * kTile * 4);
    L.ql = take((size_t)kStages * 2 * kTile * 8);
    L.nar = take((size_t)kStages * 4);    // per tile stage: accounts fit int32 (SmaAcct)
    L.ctr = take(4);
    L.total = o;
    return L;
}

// ---------------------------------------------------- EMA+OLS and Bollinger (k_ema.hip, k_boll.hip)
constexpr int kEStride = kTile + 1;  // ema buffer row stride (doubles): conflict-free columns
// Bollinger tile buffers: scanned (k+2), flagged (k+1), walked (k) and accounted (k-1, by the
// accountant wave of a split walk)
constexpr int kBollStages = 4;
// EMA+OLS runs stages of TS tiles per barrier (ema_tile_kernel): closes, returns and narrow
// flags of three stages in flight (scanned st+2, flagged st+1, walked st), drawdown tables, chain
// values and condition words of two (built / chained / flagged st+1 or st+2, read a stage later)
__host__ __device__ constexpr int ema_ct_slots(int ts) { return 3 * ts; }
__host__ __device__ constexpr int ema_slots(int ts) { return 2 * ts; }
// drawdown tables: 64-bar stages build them in the scan (three stages of buffers, as the closes),
// 128-bar stages a stage later (two)
__host__ __device__ constexpr int ema_dst_slots(int ts) { return ts == 1 ? ema_ct_slots(1) : ema_slots(ts); }
constexpr int kEmaTS = 2;  // 128-bar stages where the LDS allows (plan.cpp ema_stage_tiles)

// Trade records per lane and tile: an entry needs a bar after the previous exit and an exit a bar
// after its entry, so a tile holds at most 32 entries plus the exit of a position carried in.
constexpr int kRecCap = 33;

// Bollinger per-stage low/high staging (int32): lows[64], highs[64], 8 block minima of the lows
// then 8 block maxima of the highs, per bar the minimum low / maximum high from that bar to the
// end of its 8-bar block, and per bar the minimum low / maximum high from that bar to the end of
// the tile (SL/TP first-passage search)
constexpr int kLH = 6 * kTile + 16;

struct TileLds {
    size_t r1, r2, ct, ql, dst, stl, sth, ebuf, words, win, lev, levp, levf, lvb, rec, nrec, nar, ctr, total;
};

// kind 0 = EMA+OLS (na spans, nb windows, ts tiles per stage), 1 = Bollinger (na windows, nb ks,
// nlev SL/TP levels per side: nsl + ntp)
__host__ __device__ inline TileLds tile_lds_layout(int kind, int ring, int na, int nb, int nlev = 0,
                                                  int ts = kEmaTS) {
    TileLds L{};
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o += (bytes + 15) & ~size_t(15); return r; };
    // tile buffers: Bollinger kBollStages (one per 64-bar pipeline stage); EMA ema_ct_slots
    // for closes / returns / narrow flags and ema_slots for tables, chain values and words
    const int ns = kind == 1 ? kBollStages : ema_ct_slots(ts), nd = kind == 1 ? kBollStages : ema_dst_slots(ts);
    L.r1 = take((size_t)ring * 8);
    L.r2 = take((size_t)ring * (kind == 0 ? 8 : 16));
    L.ct = take((size_t)ns * kTile * 4);
    L.ql = take((size_t)ns * 2 * kTile * 8);
    L.dst = take((size_t)nd * kDstLevels * kTile * sizeof(Agg));
    if (kind == 1) {
        L.stl = take((size_t)ns * kLH * 4);  // lows, highs, block and in-block suffix extrema
        L.ebuf = take((size_t)nb * 8);                              // k_num^2 as doubles
        L.words = take((size_t)2 * (na * nb + 2 * na) * 8);
        L.win = take((size_t)na * 4);
        L.lev = take((size_t)2 * 2 * nlev * kTile);  // first-passage bars, [tile & 1][side][level][bar]
        L.levp = take((size_t)3 * 2 * nlev * kTile * 4);  // the levels (int32), [tile % 3][side][level][bar]
        L.levf = take((size_t)2 * nlev * 8);         // level factors per side
        L.lvb = take((size_t)(nlev + 1) * 4);        // distinct SL/TP bps, then their count
        // the finder's trade records [tile & 1][record][lane] and records per lane [tile & 1][lane]
        L.rec = take((size_t)2 * kRecCap * kTile * 2);
        L.nrec = take((size_t)2 * kTile);
        L.nar = take((size_t)ns * 4);  // per tile stage: the accountant's sums fit int32 (Acct32)
    } else {
        L.ebuf = take((size_t)ema_slots(ts) * na * kEStride * 8);
        L.words = take((size_t)ema_slots(ts) * (4 * na + 2 * nb) * 8);
        L.win = take((size_t)nb * 4);
        L.nar = take((size_t)ns * 4);  // per tile stage: the walk's accounts fit int32 (Acct32)
    }
    L.ctr = take(4);
    L.total = o;
    return L;
}

}  // namespace bt
