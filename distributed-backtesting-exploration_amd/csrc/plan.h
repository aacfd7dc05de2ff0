// plan.h — everything the host decides before a launch, as pure functions of the configuration,
// the dataset shape and a CU count (plan.cpp). No HIP call, no device state: the engine
// (engine.cpp, analysis.cpp) asks for a plan and sizes its buffers from it, the launchers
// (k_sma.hip, k_ema.hip, k_boll.hip) enqueue what it says, and tests/plan/*_driver.cpp print it without a GPU.
// The plan of an analysis call (listed at the head of analysis.cpp) also owns the layout of the
// call's device staging: the engine allocates staging_bytes, never fewer than 256 for a call it
// does not refuse, and every region the plan names lies inside them.
#pragma once
#include "internal.h"

namespace bt {

constexpr int kCusFallback = 256;  // CU count assumed when the device attribute cannot be read
constexpr size_t kCuLdsBytes = 160 * 1024;

// The axes of a configuration in Grid order (a, b, c, d), each with its name and the range its
// values must lie in. Returns how many the strategy has (0: unknown strategy).
struct AxisSpec {
    const int32_t* v;
    int32_t n;
    const char* what;
    int32_t lo, hi;
};
int config_axes(const bt_config& c, AxisSpec ax[4]);

// Validates the parameter grid of a configuration and fills the host-side fields of `g`: strategy,
// axis sizes, n_params, band_bps / k_den, wmax, ring, kn2 and kmin_idx (not the device pointers,
// sqrt_ann or ablate). Returns "" or the reason the grid is refused.
std::string plan_grid(const bt_config& c, Grid& g);

// What one run is launched with.
struct LaunchPlan {
    int32_t G;                     // bar segments per symbol (1 = no split)
    int32_t burn_tiles;            // tiles walked before a speculative segment's first bar
    int32_t grid_y;                // y-blocks per symbol
    int32_t block;                 // threads per block
    size_t lds;                    // dynamic LDS bytes per block
    int32_t dedicated, one_trip;   // SMA: helper wave runs the tile scan; 16-wave compare loop
    int32_t ts;                    // EMA+OLS: tiles per stage
    int32_t xw, lpw;               // tile kernels: task-only waves, lanes per parameter wave
    int32_t split_grp;             // Bollinger: parameter wave whose walk is split (-1: none)
    uint32_t wmap;                 // Bollinger: hardware wave -> role, 4 bits each
    // segment buffers of a split run (all 0 when G == 1)
    size_t seg_slots;              // SegRec slots of SegArgs::rec, SMA position planes included
    size_t pos_off, pos_bytes;     // SMA: SegArgs::pos, in bytes from SegArgs::rec, and its size
    size_t ema_doubles;            // EMA+OLS: doubles of SegArgs::ema
    bool topk_lds_free;            // the top-k chain's histograms must take no LDS
    // The run may execute beside the run before it and the run after it (consecutive runs on two
    // streams, engine.cpp run_impl): it touches nothing single-buffered (segment records of a
    // split run, parity sums and trades, profiling stamps), the engine owns its streams,
    // bt_set_run_overlap has not switched it off, and it has more blocks than the device holds at
    // once, so that there is a last round whose freed slots the next run can fill.
    bool overlap;
};

struct RunShape {
    int32_t n_sym, max_bars;       // symbols of the dataset and the longest one's bars
    bool parity;
    int32_t seg_req, burn_req;     // bt_set_segments: 0 = automatic / default
    int cus;                       // compute units of the device
    bool own_stream = true;        // the engine made its stream (false: bt_config.stream, the caller's)
    bool overlap_on = true;        // bt_set_run_overlap
};

// `ax0`: the host copy of the grid's first axis (Grid::a; the EMA burn-in follows its spans).
LaunchPlan plan_launch(const Grid& g, const int32_t* ax0, const RunShape& r);

// The one way a staging layout is made: regions taken one after the other, each starting on a
// 256-byte boundary. take() returns the region's offset; `end` is the bytes carved so far.
constexpr size_t kStagingAlign = 256;
struct Carve {
    size_t end = 0;
    size_t take(size_t bytes) {
        const size_t at = end;
        end = at + (bytes + kStagingAlign - 1) / kStagingAlign * kStagingAlign;
        return at;
    }
    size_t staging_bytes() const { return end > kStagingAlign ? end : kStagingAlign; }
};

// What a replay (k_replay.hip, bt_replay) of n lanes is launched with. The requests go through
// the device in chunks of lanes_per_chunk (the last one shorter): chunk c holds lanes
// [c * lanes_per_chunk, min(n, (c + 1) * lanes_per_chunk)), every lane exactly once. A chunk's
// staging is bounded by the budget: as many lanes as fit, and one lane always fits the default
// budget (a lane of the longest symbol, 2^22 bars, with its curves and a full trade list needs
// 37.7 + 134 MB).
constexpr size_t kReplayBudget = 256u << 20;
struct ReplayPlan {
    int64_t dcap;                  // trade slots per device row: a lane closes at most one trade per bar
    int64_t pitch;                 // elements per device curve row (0 without curves)
    int32_t lanes_per_chunk, chunks;
    size_t o_lane, o_sum, o_trades, o_equity, o_pos;  // the regions of a chunk (o_equity, o_pos:
                                   // empty when that curve is not wanted)
    size_t staging_bytes;          // of a full chunk
};
// `W`: bars of the longest requested symbol; `budget_req`: 0 = kReplayBudget (tests only: the ABI
// has no setter).
ReplayPlan plan_replay(int32_t n, int32_t W, int32_t trade_cap, int64_t stride, bool equity, bool pos,
                       size_t budget_req = 0);

// What a reduction of an S x P summary matrix is launched with (k_surface.hip launch_surface).
// Lanes run along p: grid x tiles the parameters in blocks of `block` threads, grid y cuts the
// rows into `chunks`. Chunk c holds rows_per_chunk + (c < rows_rem) rows, starting at row
// c * rows_per_chunk + min(c, rows_rem): every row exactly once, no chunk empty while S > 0.
struct SurfacePlan {
    int32_t block;                 // threads per block of the pass kernel (a multiple of 64)
    int32_t p_blocks;              // blocks along p
    int32_t chunks;                // row chunks (1 with no rows)
    int32_t rows_per_chunk, rows_rem;
    int32_t p_tiles;               // 64-lane tiles of a row: per-row best partials
    int32_t fold_ways;             // partials left by the first of two fold steps (0: one step)
    size_t partial_bytes;          // chunk aggregates: chunks x P bt_param_agg
    size_t fold_bytes;             // the first fold step's output: fold_ways x P bt_param_agg
    size_t best_partial_bytes;     // tile winners: S x p_tiles bt_topk_rec
    // staging: the three work regions, then agg[P] and best[S] next to each other (one copy
    // brings both back), then the matrix and ids a staged call (bt_surface_of) uploads
    size_t o_partial, o_fold, o_best_partial, o_agg, o_best, o_sum, o_ids;
    size_t staging_bytes;
};
// `chunks_req`: bt_set_surface_chunks (0 = automatic); `staged`: the layout holds the S x P matrix
// and the S ids too.
SurfacePlan plan_surface(int32_t S, int32_t P, int cus, int32_t chunks_req, bool staged = false);

// What a walk-forward evaluation (k_walkfwd.hip, bt_walk_forward) of S rows x P params x K folds is
// launched with. The rows are processed in chunks of rows_per_chunk (the last one shorter): chunk c
// holds rows [c * rows_per_chunk, min(S, (c + 1) * rows_per_chunk)), every row exactly once. A
// chunk's device staging is the bounds, its fold records [rows][K][P] and its steps (sized for the
// most a call can ask for, K - 1 per row), and never exceeds the budget. rows_per_chunk == 0: one
// row alone does not fit, and the call is refused.
constexpr size_t kWalkfwdBudget = 256u << 20;
struct WalkfwdPlan {
    int32_t rows_per_chunk, chunks;
    int32_t sel_block;             // threads of a selection block (a multiple of 64, at most 256)
    int32_t tiles;                 // 64-bar tiles the longest row's waves walk
    int64_t waves;                 // walk workgroups (one wave each) of a full chunk
    double fill;                   // ... in units of what the device holds at once (8 waves per SIMD)
    size_t bounds_bytes, row_bytes;  // staging: the bounds (padded), and per row of a chunk
    size_t staging_bytes;          // of a full chunk (0 with rows_per_chunk == 0)
    size_t o_rec, o_steps;         // the chunk's records and steps; the bounds lie at 0
};
// `budget_req`: bt_set_walkfwd_budget (0 = kWalkfwdBudget).
WalkfwdPlan plan_walkfwd(int32_t S, int32_t P, int32_t K, int32_t max_bars, int cus, int64_t budget_req = 0);

// What a probability of backtest overfitting (k_cscv.hip, bt_cscv / bt_cscv_of) of G groups x P
// lanes x K folds is launched with. C = binom(K, K/2) combinations in `pairs` = C / 2 pairs (c,
// C - 1 - c), one thread each: masks[q] is combination q's K-bit word (bit K - 1 clear), in
// increasing numeric order. The groups go through the device in chunks of rows_per_chunk whole
// rows (the last one shorter), bounded by the walk-forward budget: per row its fold records (the
// walk's [K][P] or a staged call's [P][K]), the packed sums [P][K + 1] (a lane's K folds, then its
// total), the K return-bar counts, the group record, the histogram and, when asked for, C picks.
// rows_per_chunk == 0: one row alone does not fit, and the call is refused. A chunk is cut into
// launches of at most `work` cells, a cell being one (row, pair, lane): rows_per_launch whole rows
// with every pair while a row has at most `work` cells, else one row and pairs_per_launch pairs
// (a multiple of the block above one block), so that no single kernel runs long.
constexpr int64_t kCscvWork = 6000000000LL;    // 0.22 s at the measured rate: profiles/cscv/README.md
constexpr int32_t kCscvMaxRowsPerLaunch = 65535;   // grid y
struct CscvPlan {
    int64_t C, pairs;
    std::vector<uint32_t> masks;   // [pairs]
    int32_t block;                 // threads of a combination block (a multiple of 64, at most 256)
    int32_t rows_per_chunk, chunks;
    int32_t rows_per_launch;       // whole rows per launch (1 when a row is cut)
    int64_t pairs_per_launch;      // pairs of a row per launch (`pairs` when rows are whole)
    int32_t launches_per_row;      // ceil(pairs / pairs_per_launch)
    int32_t pack_block;            // threads of a pack block (one thread per (row, lane) of a chunk)
    size_t bounds_bytes, row_bytes;
    size_t o_masks, o_rec, o_sums, o_nret, o_groups, o_hist, o_picks;   // the bounds lie at 0
    size_t staging_bytes;          // of a full chunk (0 with rows_per_chunk == 0)
};
// The first C / 2 K-bit words with K / 2 bits set, ascending (Gosper's hack); K even in [2, 20].
std::vector<uint32_t> cscv_masks(int32_t K);
// `budget_req`: bt_set_walkfwd_budget (0 = kWalkfwdBudget); `work_req`: bt_set_cscv_work (0 = kCscvWork).
CscvPlan plan_cscv(int32_t G, int32_t P, int32_t K, bool want_picks, int64_t budget_req = 0, int64_t work_req = 0);

// What the trade statistics (k_tstats.hip, bt_trade_stats) are launched with. The units of a call
// are dataset rows of P lanes each (all-lanes mode) or requested lanes (list mode), processed in
// chunks of per_chunk (the last one shorter): chunk c holds units [c * per_chunk, min(units,
// (c + 1) * per_chunk)), every unit exactly once. A chunk's device staging never exceeds the
// budget. All-lanes mode: agg[P], which the reduction accumulates across the chunks, then the
// chunk's records [rows][P]. List mode: the chunk's LaneRef, then its records. per_chunk == 0: one
// unit alone does not fit, and the call is refused. The reduction runs threads along p in blocks
// of agg_block, agg_pblocks of them, and cuts a chunk's rows into at most agg_slices slices of at
// least kTstatsSliceRows rows (grid y), each adding its part into agg with integer atomics.
constexpr size_t kTstatsBudget = 256u << 20;
constexpr int32_t kTstatsSliceRows = 64, kTstatsMaxSlices = 64;
struct TstatsPlan {
    bool list;
    int32_t per_chunk, chunks;
    int64_t waves;                 // walk workgroups (one wave each) of a full chunk
    double fill;                   // ... in units of what the device holds at once (8 waves per SIMD)
    int32_t agg_block, agg_pblocks, agg_slices;
    size_t unit_bytes;             // staging per row (P records) or per lane (LaneRef and record)
    size_t o_agg, o_lanes, o_rec;  // o_agg: all-lanes mode; o_lanes: list mode
    size_t staging_bytes;          // of a full chunk (0 with per_chunk == 0)
};
// `units`: S in all-lanes mode, n in list mode; `budget_req`: bt_set_tstats_budget (0 = kTstatsBudget).
TstatsPlan plan_tstats(int32_t units, int32_t P, bool list, int cus, int64_t budget_req = 0);

// What the net-of-costs call (k_costs.hip, bt_costs) is launched with: plan_tstats' chunks with C
// records per lane. The units of a call are dataset rows of P lanes (all-lanes mode) or requested
// lanes (list mode), processed in chunks of per_chunk (the last one shorter), every unit exactly
// once; a chunk's device staging never exceeds the budget. All-lanes mode: agg[P * C], which the
// reduction accumulates across the chunks, then the chunk's records [rows][P][C]. List mode: the
// chunk's LaneRef, then its records [lanes][C]. per_chunk == 0: one unit alone does not fit, and
// the call is refused. The reduction runs threads along q = p * C + j in blocks of agg_block,
// agg_pblocks of them, and cuts a chunk's rows into at most kCostsMaxSlices slices of at least
// kCostsSliceRows rows (grid y), each adding its part into agg with integer atomics.
constexpr size_t kCostsBudget = 256u << 20;
constexpr int32_t kCostsSliceRows = 64, kCostsMaxSlices = 64;
struct CostsPlan {
    bool list;
    int32_t C;
    int32_t per_chunk, chunks;
    int64_t waves;                 // walk workgroups (one wave each) of a full chunk
    double fill;                   // ... in units of what the device holds at once (8 waves per SIMD)
    int32_t agg_block, agg_pblocks, agg_slices;
    size_t unit_bytes;             // staging per row (P * C records) or per lane (LaneRef and C records)
    size_t o_agg, o_lanes, o_rec;  // o_agg: all-lanes mode; o_lanes: list mode
    size_t staging_bytes;          // of a full chunk (0 with per_chunk == 0)
};
// `units`: S in all-lanes mode, n in list mode; `budget_req`: bt_set_costs_budget (0 = kCostsBudget).
CostsPlan plan_costs(int32_t units, int32_t P, int32_t C, bool list, int cus, int64_t budget_req = 0);

// What the tail-risk call (k_tail.hip, bt_tail / bt_tail_of) is launched with. The units of a call
// are dataset rows of P lanes (all-lanes mode), requested lanes (list mode) or staged rows of
// increments (bt_tail_of), processed in chunks of per_chunk, every unit exactly once; a chunk's
// staging never exceeds the budget. One workgroup of `block` threads per lane: its first wave walks
// (or reads the staged row) and leaves the counted increments as int32 in the lane's row, then the
// whole workgroup selects on it. The row lives in dynamic LDS behind kTailFixedBytes of histograms
// and scratch (row_mode 1) while longest_n, the most bars a lane can count, is at most lds_row_cap,
// else in the arena (row_mode 2) in rows of `pitch` words, whole 256-byte lines. A staged call
// uploads into the arena rows whatever the home and, with row_mode 1, copies them to LDS. Regions:
// the levels [Q] int32, the chunk's LaneRef (list mode), its records, its quantile records [lanes][Q]
// and its rows. row_refused: bt_set_tail_row(e, 1) with a row above lds_row_cap. per_chunk == 0: one
// unit alone (need_bytes) does not fit the budget, and the call is refused.
constexpr size_t kTailBudget = 256u << 20;
constexpr size_t kTailLdsBytes = 64 * 1024;    // dynamic LDS of a workgroup: two workgroups per CU at least
constexpr size_t kTailHistBytes = BT_TAIL_LEVELS_MAX * 256 * 4;   // one 256-bin histogram per level
constexpr size_t kTailFixedBytes = kTailHistBytes + 1024;        // ... and the workgroup's scratch, in front of the row
constexpr int32_t kTailWaves = 4;
struct TailPlan {
    bool list, staged;
    int32_t Q;
    int32_t row_mode;              // 1 = LDS, 2 = arena
    bool row_refused;
    int32_t lds_row_cap;           // counted bars an LDS row holds
    int32_t block;
    size_t lds_bytes;              // dynamic LDS of a workgroup
    int64_t pitch;                 // words of an arena row (0: none)
    int32_t per_chunk, chunks;
    size_t unit_bytes, need_bytes; // staging per unit; of the fixed part and one unit
    size_t o_levels, o_lanes, o_rec, o_q, o_rows;
    size_t staging_bytes;          // of a full chunk (0 with per_chunk == 0)
};
// `units`: S in all-lanes mode, n in list mode and of a staged call; `longest_n`: the window clipped
// to the longest row, or T of a staged call; `row_req`: bt_set_tail_row; `budget_req`:
// bt_set_tail_budget (0 = kTailBudget).
TailPlan plan_tail(int32_t units, int32_t P, int32_t Q, bool list, bool staged, int32_t longest_n, int cus,
                   int32_t row_req = 0, int64_t budget_req = 0);

// What a bootstrap reality check (k_boot.hip, bt_bootstrap / bt_bootstrap_of) of n lanes in G
// groups over T bars, B resamples in blocks of L bars, is launched with. Blocks: Lp = min(L, T),
// K = ceil(T / Lp) per resample, the last one of last_len bars. A lane's prefix row of T + 1 words
// lives in LDS (row_mode 1) while kBootRedBytes + (T + 1) * 8 fit kBootLdsBytes, else in the
// staging arena (row_mode 2), in rows of `pitch` words. One workgroup of `waves` waves per lane: one
// wave walks, all of them resample (thread = resample). Held for the whole call: the start table
// [K][B] int32, the group offsets, vmax [G][B], the group records, the lane records [n], a requested
// boot [n][B] and, with a lane list, the LaneRefs and every lane's group. Per chunk of per_chunk
// lanes (the last one shorter; chunk c holds lanes [c * per_chunk, min(n, (c + 1) * per_chunk)),
// every lane exactly once): the arena rows and a staged call's increments [per_chunk][d_pitch]
// int32. The whole never exceeds the budget; need_bytes is the staging of a call with one lane per
// chunk, and per_chunk == 0 says that even that does not fit (the call is refused with need_bytes
// named). row_refused: mode 1 was asked for and the row does not fit.
constexpr size_t kBootBudget = 256u << 20;
constexpr size_t kBootLdsBytes = 64 * 1024;    // dynamic LDS of a workgroup, reduction scratch included
constexpr size_t kBootRedBytes = 512;          // the workgroup's reduction scratch, in front of the row
#ifndef BT_BOOT_WAVES
#define BT_BOOT_WAVES 4                        // measured: DESIGN.md §4.11
#endif
constexpr int32_t kBootWaves = BT_BOOT_WAVES;
constexpr int32_t kBootMaxWaves = 4;
struct BootPlan {
    int32_t T, Lp, K, last_len;
    int32_t row_mode;              // 1 = LDS, 2 = arena
    bool row_refused;
    int32_t waves, block;          // of the lane workgroup
    size_t lds_bytes;              // its dynamic LDS
    int64_t pitch, d_pitch;        // words per arena row (0 in LDS mode); int32 per staged d row (0 unless staged)
    int32_t per_chunk, chunks;
    int32_t starts_block;          // threads of a start-table block
    int64_t starts_blocks;
    int32_t finish_block;          // threads of a finish block (one block per group)
    size_t o_starts, o_goff, o_vmax, o_groups, o_rec, o_boot, o_lanes, o_gid, o_rows, o_d;
    size_t unit_bytes;             // per lane of a chunk
    size_t need_bytes;
    size_t staging_bytes;          // of a full chunk (0 with per_chunk == 0)
};
// `list`: the call has a lane list (LaneRefs and group ids are staged); `staged`: bt_bootstrap_of
// (group ids and d are staged); neither: all-lanes mode, groups of P lanes. `row_req`:
// bt_set_boot_row; `budget_req`: bt_set_boot_budget (0 = kBootBudget).
BootPlan plan_boot(int64_t n, int64_t G, int32_t T, int32_t B, int32_t L, bool list, bool staged, bool want_boot,
                   int cus, int32_t row_req = 0, int64_t budget_req = 0);

// What a drawdown bootstrap (k_ddboot.hip, bt_drawdown_boot / bt_drawdown_boot_of) of n lanes over
// T bars, B resamples in blocks of L bars, Q levels and R limits, is launched with. The blocks are
// plan_boot's: Lp, K, last_len; two_tables: last_len differs from Lp and K > 1, so that the last
// block needs a table of its own. A lane's row is its prefix row of T + 1 words, then one or two
// tables of T entries of kDdEntryBytes (r_w1, r_w2: bytes from the row's start; equal with one
// table). It lives in dynamic LDS behind kDdFixedBytes of histograms and scratch (row_mode 1) while
// it fits kDdLdsBytes, a CU's whole LDS (above 64 KB the launcher asks for it with
// hipFuncSetAttribute, and the CU then holds one workgroup: measured 3.5 times faster than arena
// rows on a config-2 row of 80 KB), else in the arena (row_mode 2) in rows of
// `pitch` bytes, whole 256-byte lines. row_refused: bt_set_ddboot_row(e, 1) with a row that does
// not fit.
// With Q > 0 the lane's B values stay for the selection: in its row of raw when raw is wanted, else
// in LDS behind the row while they fit the same limit (l_vals: bytes from the start of LDS, 0: not
// there), else in an arena row of v_pitch words. One workgroup of `block` threads per lane. Held
// for the whole call: the start table [K][B] int32, the levels and the limits. Per chunk of
// per_chunk lanes (the last one shorter; chunk c holds lanes [c * per_chunk, min(n, (c + 1) *
// per_chunk)), every lane exactly once): the LaneRefs (list mode), the records, the quantiles, the
// reach counts, a requested raw, the arena rows, the value rows and a staged call's increments
// [per_chunk][d_pitch] int32. The whole never exceeds the budget; need_bytes is the staging of a call
// with one lane per chunk, and per_chunk == 0 says that even that does not fit (the call is refused
// with need_bytes named).
constexpr size_t kDdBudget = 256u << 20;
constexpr size_t kDdLdsBytes = 160 * 1024;     // dynamic LDS of a workgroup at most: the CU's
constexpr size_t kDdFixedBytes = kTailHistBytes + 1024;   // the histograms and the workgroup's scratch
constexpr size_t kDdEntryBytes = 24;           // a table entry: (h, l, dd)
constexpr int32_t kDdWaves = 4;
constexpr int64_t kDdScanCost = 8;             // a 64-bar tile scanned with the operator, in serial steps
// The table of `len`-bar blocks over T bars by nthr threads: a wave scans a chunk (true) or a thread
// walks one. nc chunks hold a start; the longer critical path loses.
BT_HD inline bool dd_wave_scan(int32_t T, int32_t len, int32_t nthr) {
    const int64_t nc = ((int64_t)T + len - 1) / len, nw = nthr / 64;
    const int64_t serial = (int64_t)len * ((nc + nthr - 1) / nthr);
    const int64_t scan = ((nc + nw - 1) / nw) * (((int64_t)len + 63) / 64) * kDdScanCost;
    return scan < serial;
}
struct DdPlan {
    int32_t T, Lp, K, last_len;
    bool two_tables;
    bool scan1, scan2;             // dd_wave_scan of the two tables, as the kernel itself evaluates it: for the
                                   // plan driver and the tests, nothing is launched by them
    int32_t row_mode;              // 1 = LDS, 2 = arena
    bool row_refused;
    size_t r_w1, r_w2, row_bytes;
    int32_t block;
    size_t lds_bytes, l_vals;      // dynamic LDS of a workgroup
    int64_t pitch, d_pitch, v_pitch;
    int32_t per_chunk, chunks;
    int32_t starts_block;          // threads of a start-table block
    int64_t starts_blocks;
    size_t o_starts, o_levels, o_limits, o_lanes, o_rec, o_q, o_reach, o_raw, o_rows, o_vals, o_d;
    size_t unit_bytes;             // per lane of a chunk
    size_t need_bytes;
    size_t staging_bytes;          // of a full chunk (0 with per_chunk == 0)
};
// `list`: the call has a lane list; `staged`: bt_drawdown_boot_of; neither: all-lanes mode. `row_req`:
// bt_set_ddboot_row; `budget_req`: bt_set_ddboot_budget (0 = kDdBudget). `cus` is taken as every
// plan function takes it and not used: one workgroup per lane whatever the device.
DdPlan plan_ddboot(int64_t n, int32_t T, int32_t B, int32_t L, int32_t Q, int32_t R, bool list, bool staged,
                   bool want_raw, int cus, int32_t row_req = 0, int64_t budget_req = 0);

// What a portfolio (k_portfolio.hip, bt_portfolio) of n entries over T bars is launched with. The
// walk's workgroups (one wave per entry) add into R replicas of two per-bar accumulators of
// `pitch` 8-byte words each (entry b uses replica b % R), so that the waves, which all start at
// tile 0 together, do not meet on one row. R is the largest power of two that is at most
// kPortfolioMaxReplicas, at most n, and whose accumulators fit kPortfolioAccBudget; at least 1
// (T = 2^22: 64 MB). The staging is O(R * T + n), never n * T: the entry descriptors, the two
// accumulators, then the four output rows and the summary next to each other (one copy brings
// them back).
constexpr int32_t kPortfolioMaxReplicas = 64;
constexpr size_t kPortfolioAccBudget = 64u << 20;
struct PortfolioPlan {
    int32_t R;                     // accumulator replicas
    int32_t finish_block;          // threads of the finish block (a multiple of 64, at most 1024)
    int64_t pitch;                 // words per accumulator row: T rounded up to a 64-bar tile
    int32_t tiles;                 // 64-bar tiles of the T bars
    double fill;                   // walk waves in units of what the device holds at once (8 per SIMD)
    size_t o_lanes, o_acc_pnl, o_acc_cnt, o_pnl, o_equity, o_long, o_short, o_sum;
    size_t acc_bytes;              // the two accumulators, o_acc_pnl onward: zeroed before the walk
    size_t out_bytes;              // o_pnl to the end of the summary
    size_t staging_bytes;
};
// `replicas_req`: bt_set_portfolio_replicas (0 = the rule above; else that many, at most
// kPortfolioMaxReplicas and halved until the accumulators fit the budget); `budget_req`: 0 =
// kPortfolioAccBudget (tests only: the ABI has no setter).
PortfolioPlan plan_portfolio(int32_t n, int32_t T, int cus, int32_t replicas_req = 0, size_t budget_req = 0);

// What a Gram product (k_gram.hip, bt_covariance / bt_gram_of) of n lanes over T bars is launched
// with. D holds one row of `pitch` int32 per lane (T rounded up to 64; the padding is zero) and the
// product runs one wave per 16 x 16 tile of the upper triangle (rows past n read as zero) and bar
// chunk. A small n with a long T has few tiles (64 lanes: 10), so the bars are cut into `chunks`
// chunks of chunk_bars (a multiple of 64, the last one shorter; none empty) until the device holds
// kGramWavesPerCu waves per CU, a chunk keeping at least kGramMinChunkBars bars and the partials
// kGramPartialBudget bytes; a large n gets one chunk. The staging: the lane descriptors, D, the
// chunk partials, then gram[n][n] and sums[n] next to each other (one copy brings both back).
constexpr int kGramWavesPerCu = 8;
constexpr int32_t kGramMinChunkBars = 512;
constexpr size_t kGramPartialBudget = 64u << 20;
constexpr size_t kGramStagingMax = 256u << 20;   // the call is refused above it
struct GramPlan {
    int32_t nt, tiles;             // 16-row tiles along n; tiles of the upper triangle
    int32_t chunks, chunk_bars;
    int32_t fold_block;            // threads of a fold block (a multiple of 64)
    int64_t pitch;
    double fill;                   // product waves in units of kGramWavesPerCu per CU
    size_t o_lanes, o_d, o_partial, o_gram, o_sums;
    size_t d_bytes;                // D: zeroed before the walk or the upload
    size_t out_bytes;              // o_gram to the end of the sums
    size_t staging_bytes;
};
// `split_req`: bt_set_gram_split (0 = the rule above; else that many chunks, at most one per 64 bars).
GramPlan plan_gram(int32_t n, int32_t T, int cus, int32_t split_req = 0);

// The staging of a top-k chain over a caller's S x P records (k_topk.hip, bt_topk_of): what the
// call uploads (order keys, summaries, one SymDesc per row) and a TopkWork of its own, so that the
// engine's own top-k buffers are never touched: the 4,096-bin histogram, the selection state,
// the two counts, kTopkCap indices above the selected prefix and kTopkCap candidates, and the
// result with its count in front (kTopkMax + 1 records).
struct TopkOfPlan {
    size_t o_key, o_sum, o_syms;
    size_t o_hist, o_state, o_counts, o_above, o_cand, o_out;
    size_t staging_bytes;
};
TopkOfPlan plan_topk_of(int32_t S, int32_t P);

}  // namespace bt
