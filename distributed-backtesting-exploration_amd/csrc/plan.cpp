// plan.cpp — the host's launch decisions (plan.h): grid validation and ring sizing, block shapes,
// bar segments, dynamic LDS and segment buffer sizes, and the chunks and staging layouts of the
// analysis calls. Pure functions: no HIP call, no device state; the profiling build's environment
// overrides sit next to the rules they override.
#include "plan.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "batch.h"
#include "cscv.h"
#include "csv.h"
#include "lds_layout.h"

namespace bt {

namespace {

constexpr int kDefaultBurnTiles = 64;  // tile kernels
constexpr int kSmaBurnTiles = 2;

uint32_t next_pow2(uint32_t x) {
    uint32_t r = 1;
    while (r < x) r <<= 1;
    return r;
}

size_t ema_lds_bytes(const Grid& g, int ts) { return tile_lds_layout(0, g.ring, g.na, g.nb, 0, ts).total; }

}  // namespace

// ------------------------------------------------------------------------ grid configuration
int config_axes(const bt_config& c, AxisSpec ax[4]) {
    switch (c.strategy) {
        case BT_SMA_CROSS:
            ax[0] = {c.fast, c.n_fast, "fast", 1, kMaxBars};
            ax[1] = {c.slow, c.n_slow, "slow", 1, kMaxBars};
            return 2;
        case BT_EMA_OLS:
            ax[0] = {c.span, c.n_span, "span", 1, kMaxBars};
            ax[1] = {c.ols, c.n_ols, "ols", 1, 1 << 16};
            return 2;
        case BT_BOLL:
            ax[0] = {c.bwin, c.n_bwin, "bwin", 1, 1 << 16};
            ax[1] = {c.k_num, c.n_k, "k_num", 0, 1 << 20};
            ax[2] = {c.sl_bps, c.n_sl, "sl_bps", 0, 9999};
            ax[3] = {c.tp_bps, c.n_tp, "tp_bps", 0, 9999};
            return 4;
        default:
            return 0;
    }
}

std::string plan_grid(const bt_config& c, Grid& g) {
    AxisSpec ax[4];
    const int nax = config_axes(c, ax);
    if (nax == 0) return "unknown strategy";
    for (int i = 0; i < nax; ++i) {
        if (ax[i].n <= 0 || ax[i].v == nullptr) return std::string("empty axis: ") + ax[i].what;
        for (int32_t j = 0; j < ax[i].n; ++j)
            if (ax[i].v[j] < ax[i].lo || ax[i].v[j] > ax[i].hi)
                return std::string("value out of range on axis ") + ax[i].what + ": " + std::to_string(ax[i].v[j]);
    }
    auto amax = [&](int i) { return *std::max_element(ax[i].v, ax[i].v + ax[i].n); };
    g.strategy = c.strategy;
    g.na = ax[0].n;
    g.nb = ax[1].n;
    g.nc = nax > 2 ? ax[2].n : 1;
    g.nd = nax > 3 ? ax[3].n : 1;
    switch (c.strategy) {
        case BT_SMA_CROSS:
            g.wmax = std::max(amax(0), amax(1));
            // prefix ring, a power of two: the longest window back from the tile whose keys are
            // built, with three tiles in flight (k_sma.hip: scan k+2, keys k+1, compare k)
            g.ring = (int32_t)next_pow2((uint32_t)g.wmax + 3 * kTile);
            if (sma_lds_layout(g.ring, g.na + g.nb).total > kCuLdsBytes)
                return "SMA grid needs more LDS than a CU has (windows too long)";
            break;
        case BT_EMA_OLS:
            if (c.band_bps < 0 || c.band_bps >= 10000) return "band_bps out of range";
            if (c.n_span > 64) return "EMA grid: at most 64 spans (one helper lane per span)";
            g.band_bps = c.band_bps;
            g.wmax = amax(1);
            // prefix ring, rounded up to a multiple of the tile: a window back from the stage being
            // flagged, which ends two 128-bar stages (four tiles) before the last scanned bar
            // (k_ema.hip ema_tile_kernel)
            g.ring = (g.wmax + 5 * kTile - 1) / kTile * kTile;
            if (ema_lds_bytes(g, 1) > kCuLdsBytes) return "EMA grid needs more LDS than a CU has (OLS windows too long)";
            break;
        default: {
            if (c.k_den < 1 || c.k_den > (1 << 20)) return "k_den out of range";
            g.k_den = c.k_den;
            g.wmax = amax(0);
            // z tests D^2 kd^2 vs kn^2 Q with D^2, Q < w^2 2^62: exact in int128 while
            // w * max(k_num, k_den) < 2^32 (spec §4, oracle/oracle.c orc_boll)
            const int64_t kmax = std::max<int64_t>(c.k_den, amax(1));
            if ((int64_t)g.wmax * kmax >= (1LL << 32)) return "Bollinger grid outside the exact int128 range (window * k >= 2^32)";
            // prefix rings: the longest window + three tiles in flight (k_ema.hip, k_boll.hip: scanned k+2,
            // flagged k+1, walked k), rounded up to a multiple of the tile
            g.ring = (g.wmax + 4 * kTile - 1) / kTile * kTile;
            for (int q = 0; q < 8; ++q) {
                const int64_t kn = q < c.n_k ? c.k_num[q] : 0;
                g.kn2[q] = (double)(kn * kn);  // exact: kn <= 2^20
            }
            g.kmin_idx = (int32_t)(std::min_element(c.k_num, c.k_num + c.n_k) - c.k_num);
            if (tile_lds_layout(1, g.ring, g.na, g.nb, g.nc + g.nd).total > kCuLdsBytes)
                return "Bollinger grid needs more LDS than a CU has (windows too long)";
            break;
        }
    }
    const int64_t P = (int64_t)g.na * g.nb * g.nc * g.nd;
    if (P <= 0 || P > (1 << 20)) return "parameter grid too large";
    g.n_params = (int32_t)P;
    return "";
}

// -------------------------------------------------------------------------------- launch plans
namespace {

// Segment records of a split run: one per (segment, symbol, param).
size_t seg_records(const LaunchPlan& pl, const Grid& g, const RunShape& r) {
    return pl.G > 1 ? (size_t)pl.G * r.n_sym * g.n_params : 0;
}

struct SmaShape {
    int pw;                           // parameter waves per block
    int dedicated;                    // 1: an extra helper wave runs the tile scan
    int block, gy;                    // threads per block, y-blocks per symbol
};

// Block shape: one block per symbol when the parameters fit (<= 15 parameter waves + a helper,
// or exactly 16 waves with the scan folded into the last parameter wave), otherwise the fewest
// equal y-blocks; each y-block recomputes the tile scan and keys, so splits are avoided.
SmaShape sma_shape(int P) {
    const int need = (P + 63) / 64;
    SmaShape s;
    if (need == 16) {
        s.pw = 16;
        s.dedicated = 0;
    } else {
        const int nby = (need + 14) / 15;
        s.pw = (need + nby - 1) / nby;
        s.dedicated = 1;
    }
    s.block = 64 * (s.pw + s.dedicated);
    s.gy = (P + 64 * s.pw - 1) / (64 * s.pw);
    return s;
}

// Bar segments for a shard of one-block-per-CU symbols (16-wave blocks: config 5) that fills the
// GPU only a few times over: block times vary with each symbol's trade count, so the launch ends
// with the CU whose few blocks took longest (config 5's 1,250-symbol 8-GPU shard: 4.9 blocks per
// CU, 121 us per symbol against 107 at 10,000 symbols). Cutting each symbol into G segments gives
// G times as many, shorter blocks. A segment costs its burn-in tiles and a ring-only lookback
// over the longest window (about a twentieth of a tile each): G is kept where that stays under 2 %
// of a segment. Shapes of several blocks per CU (config 2) keep G = 1.
int32_t sma_auto_segments(int32_t n_sym, const SmaShape& sh, int32_t max_bars, int32_t wmax,
                          int32_t burn_tiles, int cus) {
    if (n_sym <= 0) return 1;
    if (sh.block <= 512) return 1;
    // enough segment blocks for ~kSegRounds rounds of one block per CU (config 5's 1,250-symbol
    // shard, 4.9 rounds unsplit, round 4: G = 3 / 4 / 5 / 6 / 8 -> 135.0 / 133.5-134.0 /
    // 132.4-132.5 / 132.0 / 132.5 ms; each segment adds one 128-B record per parameter)
    constexpr double kSegRounds = 28.0;
    const double rounds = (double)n_sym * sh.gy / cus;
    if (rounds >= kSegRounds) return 1;
    int G = std::min(8, (int)std::ceil(kSegRounds / rounds));
    const int ntiles = (max_bars + kTile - 1) / kTile;
    const int lookback = (wmax - 1 + kTile - 1) / kTile;
    while (G > 1 && burn_tiles + 0.05 * lookback > 0.02 * ntiles / G) --G;
    return G;
}

void plan_sma(const Grid& g, const RunShape& r, LaunchPlan& pl) {
    const SmaShape sh = sma_shape(g.n_params);
    pl.burn_tiles = r.burn_req > 0 ? r.burn_req : kSmaBurnTiles;
    if (!r.parity)
        pl.G = r.seg_req > 0 ? r.seg_req
                             : sma_auto_segments(r.n_sym, sh, r.max_bars, g.wmax, pl.burn_tiles, r.cus);
    pl.grid_y = sh.gy;
    pl.block = sh.block;
    pl.dedicated = sh.dedicated;
    pl.lds = sma_lds_layout(g.ring, g.na + g.nb).total;
    // blocks of more than 8 waves (config 5: one 16-wave block per CU) hide little LDS latency:
    // their reversal loop issues all of an iteration's reads before one wait
    pl.one_trip = sh.block > 512;
#ifdef BT_PROFILING
    if (BT_ABL(g, 128)) pl.lds = std::max(pl.lds, (size_t)(g.ablate & 256 ? 80 : 60) * 1024);  // occupancy probe
    if (const char* v = getenv("BT_ONE_TRIP")) pl.one_trip = atoi(v) != 0;  // tuning aid
#endif
    // one SegRec slot per SmaSegRec, then the int8 start / end position planes
    const size_t nrec = seg_records(pl, g, r);
    pl.pos_off = nrec * sizeof(SegRec);
    pl.pos_bytes = 2 * nrec;
    pl.seg_slots = nrec + (pl.pos_bytes + sizeof(SegRec) - 1) / sizeof(SegRec);
}

// ------------------------------------------------------------------------- tile kernel plans
// Extra task-only waves per block (they take condition-word tasks only). The EMA kernel has one
// parameter wave per symbol on config 3 and is latency-bound at ~1.5 waves per SIMD: two extra
// waves take 4.96 -> 3.68 ms, four (with the parameter wave walking only, at raised priority)
// 3.32 ms, five 3.20 ms (8 waves: two blocks per CU still fit); six no longer fit two blocks per
// CU (5.0 ms). The Bollinger kernel runs 5 waves x 2 blocks per CU and its ~120 VGPRs cap a
// CU at 16 waves: two task-only waves, with the parameter waves then walking only, take config 4
// 12.3 -> 12.0 ms (250 symbols: 9.95 -> 9.76 ms); four no longer fit two blocks (19.4 ms).
int tile_param_waves(int need, int cap) {
    int pw = std::min(need, cap);
#ifdef BT_PROFILING
    if (const char* v = getenv("BT_PW")) pw = std::max(1, std::min(atoi(v), pw));  // tuning aid
#endif
    return pw;
}

int tile_extra_waves(int used, int x) {
#ifdef BT_PROFILING
    if (const char* v = getenv("BT_XW")) x = atoi(v);  // tuning aid
#endif
    return std::max(0, std::min(x, 16 - used));
}

int tile_lanes_per_wave() {
    int l = 64;
#ifdef BT_PROFILING
    if (const char* v = getenv("BT_LPW")) l = std::max(1, std::min(atoi(v), 64));  // tuning aid
#endif
    return l;
}

// Hardware wave -> role of a Bollinger block (k_boll.hip boll_tile_kernel wave_map). Hardware wave w
// runs on SIMD w % 4, so waves w and w + 4 share one: each busy parameter wave (the walks, the
// busiest first) gets a task-only wave as its partner (task waves take fewer tasks when their
// SIMD is busy), the lightest parameter wave the helper, and the accountant of a split walk a
// light parameter wave. Identity for other block shapes.
uint32_t boll_wave_map(int pw, int nsplit, int xw) {
    uint32_t m = 0;
    for (int w = 0; w < 8; ++w) m |= (uint32_t)w << (4 * w);
    const int nw = pw + 1 + nsplit + xw;
    if (nw == 8 && pw == 4) {
        // logical roles: 0-3 parameter groups, 4 helper, then the accountant, then tasks
        const int split_map[8] = {0, 1, 2, 3, 6, 7, 5, 4};
        const int plain_map[8] = {0, 1, 2, 3, 5, 6, 7, 4};
        const int* r = nsplit == 1 ? split_map : plain_map;
        m = 0;
        for (int w = 0; w < 8; ++w) m |= (uint32_t)r[w] << (4 * w);
    }
#ifdef BT_PROFILING
    if (const char* v = getenv("BT_WAVEMAP")) m = (uint32_t)strtoul(v, nullptr, 16);  // tuning aid
#endif
    return m;
}

// Split Bollinger walk (finder + accountant waves) on by default; BT_SPLIT=0 turns it off in the
// profiling build (A/B aid).
bool tile_split_walk() {
    bool on = true;
#ifdef BT_PROFILING
    if (const char* v = getenv("BT_SPLIT")) on = atoi(v) != 0;
#endif
    return on;
}

// Bar segments per symbol for a shard of n_sym symbols of a tile kernel whose blocks hold
// `helpers` waves beside the parameter waves: a shard with no more blocks than CUs leaves every
// CU one latency-bound block (config 4 on 8 GPUs: 250 symbols, 7.95 ms), so its series are cut
// into up to 4 segments, enough for two blocks per CU, each segment at least twice the burn-in
// long.
int32_t tile_auto_segments(int32_t n_sym, int32_t n_params, int32_t max_bars, int helpers,
                           int32_t burn_tiles, int cus) {
    if (n_sym <= 0) return 1;
    const int pw = std::min((n_params + 63) / 64, 1024 / 64 - helpers);
    const long long blocks = (long long)n_sym * ((n_params + 64 * pw - 1) / (64 * pw));
    if (blocks > cus) return 1;
    int G = (int)std::min<long long>(4, std::max<long long>(1, 2LL * cus / blocks));
    const int ntiles = (max_bars + kTile - 1) / kTile;
    while (G > 1 && ntiles / G < 2 * burn_tiles) --G;
    return G;
}

// The burn-in an EMA+OLS speculative segment needs for every span's fp64 chain to meet the true
// one bit for bit.
int32_t ema_burn_tiles(int32_t max_span) {
    // fp64 EMA chains started from e = c met the true ones after 131-162 bars (span 10) to
    // 11,559-13,368 bars (span 780) over 18 starts each (round-2 measurement); started from the
    // weighted-sum estimate, after at most 2.6 (span 10) to 3.8 (span 780) spans (round 3,
    // 18 starts each): 6 spans, on top of the OLS lookback tiles the chain also runs through
    return std::max(kDefaultBurnTiles, (6 * max_span + kTile - 1) / kTile);
}

// Tiles per stage of an EMA+OLS launch: 128-bar stages (TS = 2) when they keep as many blocks per
// CU as 64-bar ones (config 3: 80.2 KB vs 61.1 KB, two either way), else TS = 1.
int ema_stage_tiles(const Grid& g) {
    const size_t cu = kCuLdsBytes, l1 = ema_lds_bytes(g, 1), l2 = ema_lds_bytes(g, 2);
    return l2 <= cu && cu / l2 >= cu / l1 ? 2 : 1;
}

void plan_ema(const Grid& g, const int32_t* spans, const RunShape& r, LaunchPlan& pl) {
    int32_t maxspan = 1;
    for (int32_t i = 0; i < g.na; ++i) maxspan = std::max(maxspan, spans[i]);
    // the default burn-in lets every span's chain meet the true one; an explicit one
    // (bt_set_segments) is honoured, the fix pass covering a short one
    pl.burn_tiles = r.burn_req > 0 ? r.burn_req : ema_burn_tiles(maxspan);
    if (!r.parity)
        pl.G = r.seg_req > 0 ? r.seg_req
                             : tile_auto_segments(r.n_sym, g.n_params, r.max_bars, 2, pl.burn_tiles, r.cus);
    pl.lpw = tile_lanes_per_wave();
    const int pw = tile_param_waves((g.n_params + pl.lpw - 1) / pl.lpw, 1024 / 64 - 2);
    pl.xw = tile_extra_waves(pw + 2, 5);
    pl.grid_y = (g.n_params + pl.lpw * pw - 1) / (pl.lpw * pw);
    pl.block = 64 * (pw + 2 + pl.xw);
    pl.ts = ema_stage_tiles(g);
    pl.lds = ema_lds_bytes(g, pl.ts);
    pl.seg_slots = seg_records(pl, g, r);
    pl.ema_doubles = pl.G > 1 ? (size_t)pl.G * r.n_sym * kEmaSegStride : 0;
    // the chain's histograms take no LDS beside a strategy kernel whose blocks fill a CU's
    // (128-bar stages: k_topk.hip topk_hist_global)
    pl.topk_lds_free = pl.ts == 2;
}

void plan_boll(const Grid& g, const RunShape& r, LaunchPlan& pl) {
    pl.burn_tiles = r.burn_req > 0 ? r.burn_req : kDefaultBurnTiles;
    // the automatic count assumes the default burn-in, whatever was requested
    if (!r.parity)
        pl.G = r.seg_req > 0 ? r.seg_req
                             : tile_auto_segments(r.n_sym, g.n_params, r.max_bars, 1, kDefaultBurnTiles, r.cus);
    pl.lpw = tile_lanes_per_wave();
    const int pw = tile_param_waves((g.n_params + pl.lpw - 1) / pl.lpw, 1024 / 64 - 1);
    pl.grid_y = (g.n_params + pl.lpw * pw - 1) / (pl.lpw * pw);
    // Split walk: the parameter wave holding the smallest z threshold (lanes run k-major) trades
    // the most, and its lanes' serial trade chains set the tile time (config 4: 7.1 walk
    // iterations per tile against 1.0-4.3 for the other waves), so that wave only finds trades
    // and an accountant wave keeps their accounts a tile later.
    if (tile_split_walk() && pw >= 2 && pl.grid_y == 1) {
        const long long per_k = (long long)g.na * g.nc * g.nd;  // lanes per z threshold
        const int grp = (int)((g.kmin_idx * per_k) / pl.lpw);
        if (grp < pw) pl.split_grp = grp;
    }
    const int nsplit = pl.split_grp < 0 ? 0 : 1;
    const int base = pw + 1 + nsplit;
    // at most one block per CU (config 4 on 8 GPUs: 250 symbols) leaves wave slots free: four
    // task-only waves (8.17 -> 7.90 ms vs two); otherwise as many as keep the block at 8 waves,
    // so two blocks share a CU at <= 128 VGPRs (config 4: three, 9.65 -> 9.51 ms; four 15.8 ms)
    const bool sparse = (long long)r.n_sym * pl.grid_y * pl.G <= r.cus;
    pl.xw = tile_extra_waves(base, sparse ? 4 : std::max(2, std::min(3, 8 - base)));
    pl.block = 64 * (base + pl.xw);
    pl.lds = tile_lds_layout(1, g.ring, g.na, g.nb, g.nc + g.nd).total;
    pl.wmap = boll_wave_map(pw, nsplit, pl.xw);
    pl.seg_slots = seg_records(pl, g, r);
}

// The run has more blocks than the device can hold at once (LDS and a CU's 32 wave slots bound a
// CU's blocks from above; registers may lower it further): only then do blocks queue behind
// occupied slots, and the next run's blocks fill the slots the last round frees. A run whose
// blocks are all resident together has no such queue: the next run's first blocks would only share
// a CU's issue slots with this run's stragglers (config 3 at 500 symbols, one round of two blocks
// per CU, measured +2.3 % overlapped; config 4 at 2,000 symbols, 3.9 rounds, -1.9 %).
bool several_rounds(const LaunchPlan& pl, const RunShape& r) {
    const long long waves = std::max(1, pl.block / 64);
    const long long by_lds = pl.lds ? (long long)(kCuLdsBytes / pl.lds) : 32;
    const long long per_cu = std::max<long long>(1, std::min<long long>(by_lds, 32 / waves));
    return (long long)r.n_sym * pl.grid_y > per_cu * std::max(r.cus, 1);
}

}  // namespace

LaunchPlan plan_launch(const Grid& g, const int32_t* ax0, const RunShape& r) {
    LaunchPlan pl{};
    pl.G = 1;
    pl.split_grp = -1;
    switch (g.strategy) {
        case BT_SMA_CROSS: plan_sma(g, r, pl); break;
        case BT_EMA_OLS: plan_ema(g, ax0, r, pl); break;
        default: plan_boll(g, r, pl); break;
    }
    pl.overlap = pl.G == 1 && !r.parity && !BT_ABL(g, 64) && r.own_stream && r.overlap_on && several_rounds(pl, r);
    return pl;
}

// ---------------------------------------------------------------------------- run reductions
// The pass is a read-once stream of 48-B records, so it wants the whole GPU whatever P is
// (config 3 has one 64-lane tile per row): the rows are cut into enough chunks for
// kSurfaceWaves waves per SIMD. Every chunk writes one 104-B partial per parameter, a little more
// than two records' worth, so a chunk keeps at least kSurfaceMinRows rows (partials then add at most
// 104 / (16 x 48) = 14 % to the bytes moved) even when that leaves fewer waves.
SurfacePlan plan_surface(int32_t S, int32_t P, int cus, int32_t chunks_req, bool staged) {
    constexpr int kSurfaceWaves = 4, kSurfaceMinRows = 16;
    constexpr int32_t kMaxGridY = 65535;
    SurfacePlan pl{};
    S = std::max(S, 0);
    P = std::max(P, 1);
    pl.p_tiles = (P + 63) / 64;
    pl.block = 64 * std::min(pl.p_tiles, 4);
    pl.p_blocks = (P + pl.block - 1) / pl.block;
    int64_t chunks = chunks_req;
    if (chunks <= 0) {
        const int64_t waves_per_chunk = (int64_t)pl.p_blocks * (pl.block / 64);
        const int64_t want = ((int64_t)std::max(cus, 1) * 4 * kSurfaceWaves + waves_per_chunk - 1) / waves_per_chunk;
        chunks = std::min<int64_t>(want, S / kSurfaceMinRows);
    }
    chunks = std::max<int64_t>(1, std::min<int64_t>(chunks, std::min<int64_t>(S, kMaxGridY)));
    pl.chunks = (int32_t)chunks;
    pl.rows_per_chunk = S / pl.chunks;
    pl.rows_rem = S % pl.chunks;
    // the fold walks its partials one after the other (a merge has branches): past kFoldDirect
    // chunks it is cut into ~sqrt(chunks) interleaved walks whose results a second step merges
    constexpr int kFoldDirect = 16;
    if (pl.chunks > kFoldDirect) pl.fold_ways = (int32_t)std::ceil(std::sqrt((double)pl.chunks));
    pl.partial_bytes = (size_t)pl.chunks * (size_t)P * sizeof(bt_param_agg);
    pl.fold_bytes = (size_t)pl.fold_ways * (size_t)P * sizeof(bt_param_agg);
    pl.best_partial_bytes = (size_t)S * (size_t)pl.p_tiles * sizeof(bt_topk_rec);
    Carve c;
    pl.o_partial = c.take(pl.partial_bytes);
    pl.o_fold = c.take(pl.fold_bytes);
    pl.o_best_partial = c.take(pl.best_partial_bytes);
    pl.o_agg = c.take((size_t)P * sizeof(bt_param_agg));
    pl.o_best = c.take((size_t)S * sizeof(bt_topk_rec));
    pl.o_sum = c.take(staged ? (size_t)S * (size_t)P * sizeof(bt_summary) : 0);
    pl.o_ids = c.take(staged ? (size_t)S * sizeof(int32_t) : 0);
    pl.staging_bytes = c.staging_bytes();
    return pl;
}

// ------------------------------------------------------------------------------- lane replay
ReplayPlan plan_replay(int32_t n, int32_t W, int32_t trade_cap, int64_t stride, bool equity, bool pos,
                       size_t budget_req) {
    ReplayPlan pl{};
    n = std::max(n, 0);
    const size_t budget = budget_req > 0 ? budget_req : kReplayBudget;
    pl.dcap = std::max<int64_t>(0, std::min<int64_t>(trade_cap, W));
    pl.pitch = equity || pos ? std::min<int64_t>(stride, align_rows(W)) : 0;
    const size_t per_lane = sizeof(LaneRef) + sizeof(bt_summary) + (size_t)pl.dcap * sizeof(bt_trade) +
                            (equity ? (size_t)pl.pitch * 8 : 0) + (pos ? (size_t)pl.pitch : 0);
    // the five regions round up by less than kStagingAlign each: what is left holds whole lanes
    const size_t pad = 5 * kStagingAlign;
    const size_t lanes = std::min<size_t>((size_t)n, std::max<size_t>(1, budget > pad ? (budget - pad) / per_lane : 0));
    pl.lanes_per_chunk = (int32_t)lanes;
    pl.chunks = lanes ? (int32_t)(((size_t)n + lanes - 1) / lanes) : 0;
    Carve c;
    pl.o_lane = c.take(lanes * sizeof(LaneRef));
    pl.o_sum = c.take(lanes * sizeof(bt_summary));
    pl.o_trades = c.take(lanes * (size_t)pl.dcap * sizeof(bt_trade));
    pl.o_equity = c.take(equity ? lanes * (size_t)pl.pitch * 8 : 0);
    pl.o_pos = c.take(pos ? lanes * (size_t)pl.pitch : 0);
    pl.staging_bytes = c.staging_bytes();
    return pl;
}

WalkfwdPlan plan_walkfwd(int32_t S, int32_t P, int32_t K, int32_t max_bars, int cus, int64_t budget_req) {
    // one grid index per (row, param) and per (row, step)
    constexpr int64_t kMaxGrid = 1LL << 30;
    WalkfwdPlan pl{};
    S = std::max(S, 0);
    P = std::max(P, 1);
    K = std::max(K, 1);
    const size_t budget = budget_req > 0 ? (size_t)budget_req : kWalkfwdBudget;
    Carve c;
    c.take(((size_t)K + 1) * sizeof(int32_t));  // the bounds, at 0
    pl.bounds_bytes = c.end;
    const size_t rec_bytes = (size_t)K * (size_t)P * sizeof(bt_fold), step_bytes = (size_t)(K - 1) * sizeof(bt_wf_step);
    pl.row_bytes = rec_bytes + step_bytes;
    // the records and the steps each round up by less than kStagingAlign
    const size_t fixed = pl.bounds_bytes + 2 * kStagingAlign;
    int64_t rows = budget > fixed ? (int64_t)((budget - fixed) / pl.row_bytes) : 0;
    rows = std::min<int64_t>(rows, kMaxGrid / std::max(P, K));
    rows = std::min<int64_t>(rows, S);
    pl.rows_per_chunk = (int32_t)rows;
    pl.chunks = rows > 0 ? (int32_t)((S + rows - 1) / rows) : 0;
    pl.sel_block = 64 * std::min((P + 63) / 64, 4);
    pl.tiles = (std::max(max_bars, 0) + kTile - 1) / kTile;
    pl.waves = rows * P;
    pl.fill = (double)pl.waves / ((double)std::max(cus, 1) * 4 * 8);
    pl.staging_bytes = rows > 0 ? fixed + (size_t)rows * pl.row_bytes : 0;
    pl.o_rec = c.take((size_t)rows * rec_bytes);
    pl.o_steps = c.take((size_t)rows * step_bytes);
    return pl;
}

// --------------------------------------------------------------------------- overfitting (CSCV)
std::vector<uint32_t> cscv_masks(int32_t K) {
    std::vector<uint32_t> m;
    if (K < 2 || K > BT_CSCV_MAX_FOLDS || K % 2) return m;
    const int64_t pairs = cscv_combos(K) / 2;
    m.reserve((size_t)pairs);
    uint32_t v = (1u << (K / 2)) - 1;              // the smallest word with K/2 bits
    for (int64_t q = 0; q < pairs; ++q) {
        m.push_back(v);
        const uint32_t c = v & (0u - v), r = v + c;   // Gosper: the next word with as many bits
        v = (((r ^ v) >> 2) / c) | r;
    }
    return m;
}

CscvPlan plan_cscv(int32_t G, int32_t P, int32_t K, bool want_picks, int64_t budget_req, int64_t work_req) {
    CscvPlan pl{};
    G = std::max(G, 0);
    P = std::max(P, 1);
    K = std::min(std::max(K, 2), BT_CSCV_MAX_FOLDS) & ~1;
    pl.masks = cscv_masks(K);
    pl.C = cscv_combos(K);
    pl.pairs = pl.C / 2;
    pl.block = (int32_t)std::min<int64_t>(256, (pl.pairs + 63) / 64 * 64);
    pl.pack_block = 64 * std::min((P + 63) / 64, 4);
    const size_t budget = budget_req > 0 ? (size_t)budget_req : kWalkfwdBudget;
    const int64_t work = work_req > 0 ? work_req : kCscvWork;
    Carve c;
    c.take(((size_t)K + 1) * sizeof(int32_t));     // the bounds, at 0
    pl.bounds_bytes = c.end;
    pl.o_masks = c.take((size_t)pl.pairs * sizeof(uint32_t));
    const size_t rec_bytes = (size_t)K * (size_t)P * sizeof(bt_fold), sum_bytes = (size_t)P * ((size_t)K + 1) * 32,
                 nret_bytes = (size_t)K * sizeof(int32_t), hist_bytes = (2 * (size_t)P - 1) * sizeof(uint32_t),
                 pick_bytes = want_picks ? (size_t)pl.C * sizeof(bt_cscv_pick) : 0;
    pl.row_bytes = rec_bytes + sum_bytes + nret_bytes + sizeof(bt_cscv_group) + hist_bytes + pick_bytes;
    // each of the six row regions rounds up by less than kStagingAlign
    const size_t fixed = c.end + 6 * kStagingAlign;
    int64_t rows = budget > fixed ? (int64_t)((budget - fixed) / pl.row_bytes) : 0;
    rows = std::min<int64_t>(rows, (1LL << 30) / P);   // one grid index per lane of a chunk (walk, pack)
    rows = std::min<int64_t>(rows, G);
    pl.rows_per_chunk = (int32_t)rows;
    pl.chunks = rows > 0 ? (int32_t)((G + rows - 1) / rows) : 0;
    const int64_t row_cells = pl.pairs * P;
    if (row_cells <= work) {
        pl.rows_per_launch = (int32_t)std::min<int64_t>(work / row_cells, kCscvMaxRowsPerLaunch);
        pl.pairs_per_launch = pl.pairs;
    } else {
        pl.rows_per_launch = 1;
        int64_t q = std::max<int64_t>(work / P, 1);
        if (q > pl.block) q -= q % pl.block;
        pl.pairs_per_launch = q;
    }
    pl.launches_per_row = (int32_t)((pl.pairs + pl.pairs_per_launch - 1) / pl.pairs_per_launch);
    pl.staging_bytes = rows > 0 ? fixed + (size_t)rows * pl.row_bytes : 0;
    pl.o_rec = c.take((size_t)rows * rec_bytes);
    pl.o_sums = c.take((size_t)rows * sum_bytes);
    pl.o_nret = c.take((size_t)rows * nret_bytes);
    pl.o_groups = c.take((size_t)rows * sizeof(bt_cscv_group));
    pl.o_hist = c.take((size_t)rows * hist_bytes);
    pl.o_picks = c.take((size_t)rows * pick_bytes);
    return pl;
}

// --------------------------------------------------------------------------- trade statistics
TstatsPlan plan_tstats(int32_t units, int32_t P, bool list, int cus, int64_t budget_req) {
    constexpr int64_t kMaxGrid = 1LL << 30;   // one grid index per lane of a chunk
    TstatsPlan pl{};
    units = std::max(units, 0);
    P = std::max(P, 1);
    pl.list = list;
    const size_t budget = budget_req > 0 ? (size_t)budget_req : kTstatsBudget;
    pl.unit_bytes = list ? sizeof(LaneRef) + sizeof(bt_tstats) : (size_t)P * sizeof(bt_tstats);
    Carve c;
    if (list) pl.o_lanes = c.take(0);
    else pl.o_agg = c.take((size_t)P * sizeof(bt_tstats_agg));
    // the chunk's regions each round up by less than kStagingAlign
    const size_t fixed = c.end + (list ? 2 : 1) * kStagingAlign;
    int64_t per = budget > fixed ? (int64_t)((budget - fixed) / pl.unit_bytes) : 0;
    per = std::min<int64_t>(per, list ? kMaxGrid : kMaxGrid / P);
    per = std::min<int64_t>(per, units);
    pl.per_chunk = (int32_t)per;
    pl.chunks = per > 0 ? (int32_t)((units + per - 1) / per) : 0;
    pl.waves = list ? per : per * P;
    pl.fill = (double)pl.waves / ((double)std::max(cus, 1) * 4 * 8);
    pl.agg_block = 64 * std::min((P + 63) / 64, 4);
    pl.agg_pblocks = (P + pl.agg_block - 1) / pl.agg_block;
    pl.agg_slices = (int32_t)std::min<int64_t>(std::max<int64_t>((per + kTstatsSliceRows - 1) / kTstatsSliceRows, 1),
                                               kTstatsMaxSlices);
    if (list) c.take((size_t)per * sizeof(LaneRef));
    pl.o_rec = c.take((size_t)per * (list ? 1 : (size_t)P) * sizeof(bt_tstats));
    pl.staging_bytes = per > 0 ? fixed + (size_t)per * pl.unit_bytes : 0;
    return pl;
}

// ------------------------------------------------------------------------------ net of costs
CostsPlan plan_costs(int32_t units, int32_t P, int32_t C, bool list, int cus, int64_t budget_req) {
    constexpr int64_t kMaxGrid = 1LL << 30;   // one grid index per lane of a chunk
    CostsPlan pl{};
    units = std::max(units, 0);
    P = std::max(P, 1);
    C = std::min(std::max(C, 1), (int32_t)BT_COST_LEVELS_MAX);
    pl.list = list;
    pl.C = C;
    const size_t budget = budget_req > 0 ? (size_t)budget_req : kCostsBudget;
    const size_t lane_bytes = (size_t)C * sizeof(bt_cost_rec);
    const int64_t PC = (int64_t)P * C;
    pl.unit_bytes = list ? sizeof(LaneRef) + lane_bytes : (size_t)P * lane_bytes;
    Carve c;
    if (list) pl.o_lanes = c.take(0);
    else pl.o_agg = c.take((size_t)PC * sizeof(bt_cost_agg));
    // the chunk's regions each round up by less than kStagingAlign
    const size_t fixed = c.end + (list ? 2 : 1) * kStagingAlign;
    int64_t per = budget > fixed ? (int64_t)((budget - fixed) / pl.unit_bytes) : 0;
    per = std::min<int64_t>(per, list ? kMaxGrid : kMaxGrid / P);
    per = std::min<int64_t>(per, units);
    pl.per_chunk = (int32_t)per;
    pl.chunks = per > 0 ? (int32_t)((units + per - 1) / per) : 0;
    pl.waves = list ? per : per * P;
    pl.fill = (double)pl.waves / ((double)std::max(cus, 1) * 4 * 8);
    pl.agg_block = (int32_t)(64 * std::min<int64_t>((PC + 63) / 64, 4));
    pl.agg_pblocks = (int32_t)((PC + pl.agg_block - 1) / pl.agg_block);
    pl.agg_slices = (int32_t)std::min<int64_t>(std::max<int64_t>((per + kCostsSliceRows - 1) / kCostsSliceRows, 1),
                                               kCostsMaxSlices);
    if (list) c.take((size_t)per * sizeof(LaneRef));
    pl.o_rec = c.take((size_t)per * (list ? 1 : (size_t)P) * lane_bytes);
    pl.staging_bytes = per > 0 ? fixed + (size_t)per * pl.unit_bytes : 0;
    return pl;
}

// --------------------------------------------------------------------------------- tail risk
TailPlan plan_tail(int32_t units, int32_t P, int32_t Q, bool list, bool staged, int32_t longest_n, int cus,
                   int32_t row_req, int64_t budget_req) {
    (void)cus;                                     // one workgroup per lane whatever the device
    constexpr int64_t kMaxGrid = 1LL << 30;        // one grid index per lane of a chunk
    TailPlan pl{};
    units = std::max(units, 0);
    P = list || staged ? 1 : std::max(P, 1);
    Q = std::min(std::max(Q, 1), (int32_t)BT_TAIL_LEVELS_MAX);
    longest_n = std::max(longest_n, 0);
    pl.list = list, pl.staged = staged, pl.Q = Q;
    pl.lds_row_cap = (int32_t)((kTailLdsBytes - kTailFixedBytes) / 4);
    const bool fits = longest_n <= pl.lds_row_cap;
    pl.row_refused = row_req == 1 && !fits;
    pl.row_mode = row_req == 2 || !fits ? 2 : 1;
    pl.block = 64 * kTailWaves;
    pl.lds_bytes = kTailFixedBytes + (pl.row_mode == 1 ? (size_t)longest_n * 4 : 0);
    pl.pitch = pl.row_mode == 2 || staged ? std::max<int64_t>(((int64_t)longest_n + 63) / 64 * 64, 64) : 0;
    const size_t budget = budget_req > 0 ? (size_t)budget_req : kTailBudget;
    const size_t lane_bytes = sizeof(bt_tail_rec) + (size_t)Q * sizeof(bt_tail_q) + (size_t)pl.pitch * 4;
    pl.unit_bytes = (size_t)P * lane_bytes + (list ? sizeof(LaneRef) : 0);
    Carve c;
    pl.o_levels = c.take((size_t)Q * 4);
    // the chunk's four regions each round up by less than kStagingAlign
    const size_t fixed = c.end + 4 * kStagingAlign;
    pl.need_bytes = fixed + pl.unit_bytes;
    int64_t per = budget > fixed ? (int64_t)((budget - fixed) / pl.unit_bytes) : 0;
    per = std::min<int64_t>(per, kMaxGrid / P);
    per = std::min<int64_t>(per, units);
    pl.per_chunk = (int32_t)per;
    pl.chunks = per > 0 ? (int32_t)((units + per - 1) / per) : 0;
    const size_t lanes = (size_t)per * (size_t)P;
    pl.o_lanes = c.take(list ? lanes * sizeof(LaneRef) : 0);
    pl.o_rec = c.take(lanes * sizeof(bt_tail_rec));
    pl.o_q = c.take(lanes * (size_t)Q * sizeof(bt_tail_q));
    pl.o_rows = c.take(lanes * (size_t)pl.pitch * 4);
    pl.staging_bytes = per > 0 ? c.staging_bytes() : 0;
    return pl;
}

// ------------------------------------------------------------------- bootstrap reality check
BootPlan plan_boot(int64_t n, int64_t G, int32_t T, int32_t B, int32_t L, bool list, bool staged, bool want_boot,
                   int cus, int32_t row_req, int64_t budget_req) {
    (void)cus;                                     // one workgroup per lane whatever the device
    constexpr int64_t kMaxGrid = 1LL << 30;        // one grid index per lane of a chunk
    BootPlan pl{};
    n = std::max<int64_t>(n, 1);
    G = std::max<int64_t>(G, 1);
    T = std::max(T, 1), B = std::max(B, 1), L = std::max(L, 1);
    pl.T = T;
    pl.Lp = std::min(L, T);
    pl.K = (T + pl.Lp - 1) / pl.Lp;
    pl.last_len = T - (pl.K - 1) * pl.Lp;
    const size_t row_bytes = ((size_t)T + 1) * 8;
    const bool fits = kBootRedBytes + row_bytes <= kBootLdsBytes;
    pl.row_refused = row_req == 1 && !fits;
    pl.row_mode = row_req == 2 || !fits ? 2 : 1;
    pl.waves = std::min(std::max(kBootWaves, 1), kBootMaxWaves);
    pl.block = 64 * pl.waves;
    pl.lds_bytes = kBootRedBytes + (pl.row_mode == 1 ? row_bytes : 0);
    pl.pitch = pl.row_mode == 2 ? ((int64_t)T + 1 + 31) / 32 * 32 : 0;   // rows of whole 256-byte lines
    pl.d_pitch = staged ? ((int64_t)T + 63) / 64 * 64 : 0;
    pl.starts_block = 256;
    pl.starts_blocks = ((int64_t)pl.K * B + pl.starts_block - 1) / pl.starts_block;
    pl.finish_block = 256;
    const size_t budget = budget_req > 0 ? (size_t)budget_req : kBootBudget;
    Carve c;
    pl.o_starts = c.take((size_t)pl.K * (size_t)B * 4);
    pl.o_goff = c.take(((size_t)G + 1) * 4);
    pl.o_vmax = c.take((size_t)G * (size_t)B * 8);
    pl.o_groups = c.take((size_t)G * sizeof(bt_boot_group));
    pl.o_rec = c.take((size_t)n * sizeof(bt_boot_lane));
    pl.o_boot = c.take(want_boot ? (size_t)n * (size_t)B * 8 : 0);
    pl.o_lanes = c.take(list ? (size_t)n * sizeof(LaneRef) : 0);
    pl.o_gid = c.take(list || staged ? (size_t)n * 4 : 0);
    // the chunk's regions: whole 256-byte lines per lane, so they round up by nothing
    pl.unit_bytes = (size_t)pl.pitch * 8 + (size_t)pl.d_pitch * 4;
    const size_t fixed = c.end;
    pl.need_bytes = std::max(fixed + pl.unit_bytes, kStagingAlign);
    int64_t per = n;
    if (pl.need_bytes > budget) per = 0;
    else if (pl.unit_bytes > 0) per = std::min<int64_t>(n, (int64_t)((budget - fixed) / pl.unit_bytes));
    per = std::min(per, kMaxGrid);
    pl.per_chunk = (int32_t)per;
    pl.chunks = per > 0 ? (int32_t)((n + per - 1) / per) : 0;
    pl.o_rows = c.take((size_t)per * (size_t)pl.pitch * 8);
    pl.o_d = c.take((size_t)per * (size_t)pl.d_pitch * 4);
    pl.staging_bytes = per > 0 ? c.staging_bytes() : 0;
    return pl;
}

// ------------------------------------------------------------------------ drawdown bootstrap
DdPlan plan_ddboot(int64_t n, int32_t T, int32_t B, int32_t L, int32_t Q, int32_t R, bool list, bool staged,
                   bool want_raw, int cus, int32_t row_req, int64_t budget_req) {
    (void)cus;                                     // one workgroup per lane whatever the device
    constexpr int64_t kMaxGrid = 1LL << 30;        // one grid index per lane of a chunk
    DdPlan pl{};
    n = std::max<int64_t>(n, 1);
    T = std::max(T, 1), B = std::max(B, 1), L = std::max(L, 1);
    Q = std::min(std::max(Q, 0), (int32_t)BT_DD_LEVELS_MAX);
    R = std::min(std::max(R, 0), (int32_t)BT_DD_LIMITS_MAX);
    pl.T = T;
    pl.Lp = std::min(L, T);
    pl.K = (T + pl.Lp - 1) / pl.Lp;
    pl.last_len = T - (pl.K - 1) * pl.Lp;
    pl.two_tables = pl.K > 1 && pl.last_len != pl.Lp;
    pl.block = 64 * kDdWaves;
    pl.scan1 = dd_wave_scan(T, pl.Lp, pl.block);
    pl.scan2 = dd_wave_scan(T, pl.last_len, pl.block);
    const size_t table = (size_t)T * kDdEntryBytes;
    pl.r_w1 = ((size_t)T + 1) * 8;
    pl.r_w2 = pl.r_w1 + (pl.two_tables ? table : 0);
    pl.row_bytes = pl.r_w2 + table;
    const bool fits = kDdFixedBytes + pl.row_bytes <= kDdLdsBytes;
    pl.row_refused = row_req == 1 && !fits;
    pl.row_mode = row_req == 2 || !fits ? 2 : 1;
    pl.lds_bytes = kDdFixedBytes + (pl.row_mode == 1 ? pl.row_bytes : 0);
    const size_t vals_bytes = (size_t)B * 8;
    if (Q > 0 && !want_raw && pl.lds_bytes + vals_bytes <= kDdLdsBytes) pl.l_vals = pl.lds_bytes, pl.lds_bytes += vals_bytes;
    pl.pitch = pl.row_mode == 2 ? (int64_t)((pl.row_bytes + 255) / 256 * 256) : 0;
    pl.v_pitch = Q > 0 && !want_raw && pl.l_vals == 0 ? ((int64_t)B + 31) / 32 * 32 : 0;
    pl.d_pitch = staged ? ((int64_t)T + 63) / 64 * 64 : 0;
    pl.starts_block = 256;
    pl.starts_blocks = ((int64_t)pl.K * B + pl.starts_block - 1) / pl.starts_block;
    const size_t budget = budget_req > 0 ? (size_t)budget_req : kDdBudget;
    Carve c;
    pl.o_starts = c.take((size_t)pl.K * (size_t)B * 4);
    pl.o_levels = c.take((size_t)Q * 4);
    pl.o_limits = c.take((size_t)R * 8);
    pl.unit_bytes = (list ? sizeof(LaneRef) : 0) + sizeof(bt_dd_lane) + (size_t)Q * 8 + (size_t)R * 8 +
                    (want_raw ? vals_bytes : 0) + (size_t)pl.pitch + (size_t)pl.v_pitch * 8 + (size_t)pl.d_pitch * 4;
    // the chunk's eight regions each round up by less than kStagingAlign
    const size_t fixed = c.end + 8 * kStagingAlign;
    pl.need_bytes = fixed + pl.unit_bytes;
    int64_t per = budget > fixed ? (int64_t)((budget - fixed) / pl.unit_bytes) : 0;
    per = std::min(std::min(per, kMaxGrid), n);
    pl.per_chunk = (int32_t)per;
    pl.chunks = per > 0 ? (int32_t)((n + per - 1) / per) : 0;
    const size_t m = (size_t)per;
    pl.o_lanes = c.take(list ? m * sizeof(LaneRef) : 0);
    pl.o_rec = c.take(m * sizeof(bt_dd_lane));
    pl.o_q = c.take(m * (size_t)Q * 8);
    pl.o_reach = c.take(m * (size_t)R * 8);
    pl.o_raw = c.take(want_raw ? m * vals_bytes : 0);
    pl.o_rows = c.take(m * (size_t)pl.pitch);
    pl.o_vals = c.take(m * (size_t)pl.v_pitch * 8);
    pl.o_d = c.take(m * (size_t)pl.d_pitch * 4);
    pl.staging_bytes = per > 0 ? c.staging_bytes() : 0;
    return pl;
}

// ------------------------------------------------------------------------ portfolio of lanes
PortfolioPlan plan_portfolio(int32_t n, int32_t T, int cus, int32_t replicas_req, size_t budget_req) {
    PortfolioPlan pl{};
    n = std::max(n, 0);
    T = std::max(T, 1);
    const size_t budget = budget_req > 0 ? budget_req : kPortfolioAccBudget;
    pl.tiles = (T + kTile - 1) / kTile;
    pl.pitch = (int64_t)pl.tiles * kTile;
    const size_t row = (size_t)pl.pitch * 16;  // one replica of both accumulators
    int32_t R = 1;
    if (replicas_req > 0) {
        R = std::min(replicas_req, kPortfolioMaxReplicas);
        while (R > 1 && (size_t)R * row > budget) R /= 2;
    } else {
        while (R * 2 <= kPortfolioMaxReplicas && R * 2 <= n && (size_t)(R * 2) * row <= budget) R *= 2;
    }
    pl.R = R;
    pl.finish_block = (int32_t)std::min<int64_t>(pl.pitch, 1024);
    pl.fill = (double)n / ((double)std::max(cus, 1) * 4 * 8);
    Carve c;
    pl.o_lanes = c.take((size_t)n * sizeof(PfLane));
    pl.o_acc_pnl = c.take((size_t)R * (size_t)pl.pitch * 8);
    pl.o_acc_cnt = c.take((size_t)R * (size_t)pl.pitch * 8);
    pl.acc_bytes = c.end - pl.o_acc_pnl;
    pl.o_pnl = c.take((size_t)T * 8);
    pl.o_equity = c.take((size_t)T * 8);
    pl.o_long = c.take((size_t)T * 4);
    pl.o_short = c.take((size_t)T * 4);
    pl.o_sum = c.take(sizeof(bt_pf_summary));
    pl.out_bytes = pl.o_sum + sizeof(bt_pf_summary) - pl.o_pnl;
    pl.staging_bytes = c.staging_bytes();
    return pl;
}

// ------------------------------------------------------------------------ covariance of lanes
GramPlan plan_gram(int32_t n, int32_t T, int cus, int32_t split_req) {
    GramPlan pl{};
    n = std::max(n, 0);
    T = std::max(T, 0);
    pl.nt = (n + 15) / 16;
    pl.tiles = pl.nt * (pl.nt + 1) / 2;
    const int64_t groups = std::max<int64_t>(1, ((int64_t)T + kTile - 1) / kTile);  // 64-bar groups
    pl.pitch = groups * kTile;
    const size_t chunk_partial = (size_t)pl.tiles * 256 * sizeof(bt_wide);
    // as many chunks as the partial budget holds, and never more than one per group
    int64_t most = chunk_partial ? std::max<size_t>(1, kGramPartialBudget / chunk_partial) : 1;
    most = std::min<int64_t>(std::min<int64_t>(most, groups), 65535);
    int64_t chunks = 1;
    if (split_req > 0) {
        chunks = split_req;
    } else if (pl.tiles > 0) {
        const int64_t want = (int64_t)std::max(cus, 1) * kGramWavesPerCu;
        chunks = std::min<int64_t>((want + pl.tiles - 1) / pl.tiles, pl.pitch / kGramMinChunkBars);
    }
    chunks = std::max<int64_t>(1, std::min(chunks, most));
    const int64_t per = (groups + chunks - 1) / chunks;  // groups per chunk: none is empty
    pl.chunk_bars = (int32_t)(per * kTile);
    pl.chunks = (int32_t)((groups + per - 1) / per);
    pl.fold_block = 256;
    pl.fill = (double)pl.tiles * pl.chunks / ((double)std::max(cus, 1) * kGramWavesPerCu);
    Carve c;
    pl.o_lanes = c.take((size_t)n * sizeof(LaneRef));
    pl.o_d = c.take((size_t)n * (size_t)pl.pitch * sizeof(int32_t));
    pl.d_bytes = c.end - pl.o_d;
    pl.o_partial = c.take((size_t)pl.chunks * chunk_partial);
    pl.o_gram = c.take((size_t)n * (size_t)n * sizeof(bt_wide));
    pl.o_sums = c.take((size_t)n * sizeof(int64_t));
    pl.out_bytes = pl.o_sums + (size_t)n * sizeof(int64_t) - pl.o_gram;
    pl.staging_bytes = c.staging_bytes();
    return pl;
}

// ---------------------------------------------------------------------- top-k of given records
TopkOfPlan plan_topk_of(int32_t S, int32_t P) {
    TopkOfPlan pl{};
    const size_t rows = (size_t)std::max(S, 0), n = rows * (size_t)std::max(P, 1);
    Carve c;
    pl.o_key = c.take(n * sizeof(uint64_t));
    pl.o_sum = c.take(n * sizeof(bt_summary));
    pl.o_syms = c.take(rows * sizeof(SymDesc));
    pl.o_hist = c.take(4096 * sizeof(unsigned int));
    pl.o_state = c.take(4 * sizeof(unsigned long long));
    pl.o_counts = c.take(2 * sizeof(unsigned int));
    pl.o_above = c.take((size_t)kTopkCap * sizeof(unsigned long long));
    pl.o_cand = c.take((size_t)kTopkCap * sizeof(unsigned long long));
    pl.o_out = c.take(((size_t)kTopkMax + 1) * sizeof(bt_topk_rec));
    pl.staging_bytes = c.staging_bytes();
    return pl;
}

}  // namespace bt
