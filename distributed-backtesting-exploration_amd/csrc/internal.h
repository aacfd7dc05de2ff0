// internal.h — layouts shared by the host engine (engine.cpp) and the HIP kernels (k_*.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/bt.h"
#include "host_common.h"

// Profiling switches (phase ablation, s_memtime stamps, launch-shape overrides from the
// environment) exist only in the profiling build (`make PROFILING=1` -> dev/prof.so). In the
// release libbt.so BT_ABL is the constant false: no environment variable can change a result.
#ifdef BT_PROFILING
#define BT_ABL(g, bit) (((g).ablate & (bit)) != 0)
// wave priority override (tuning aid): bit 20 set -> 2-bit field at `shift` replaces `dflt`
#define BT_PRIO(g, shift, dflt) (BT_ABL(g, 1 << 20) ? (((g).ablate >> (shift)) & 3) : (dflt))
#else
#define BT_ABL(g, bit) false
#define BT_PRIO(g, shift, dflt) (dflt)
#endif
// profiling stamps: slots [0, 80) role cycles, then where each of the first kDbgBlocks blocks'
// first 8 waves ran (HW_ID | XCC_ID << 32 | 1 << 40)
constexpr int kDbgSlots = 80, kDbgBlocks = 1024;

namespace bt {

constexpr int kTile = 64;          // bars per LDS tile (one bit per bar in a 64-bit word)
constexpr int kRowAlign = 64;      // symbol rows start on 64-element boundaries in HBM

// One symbol of the HBM-resident dataset: rows of int32 ticks at `off` in every column.
struct SymDesc {
    int64_t off;
    int32_t bars;
    int32_t id;                    // global symbol id (top-k tie-break, shard-independent)
};

// Device-side view of the parameter grid (copied once per engine).
struct Grid {
    int32_t strategy;
    int32_t n_params;
    int32_t na, nb, nc, nd;        // axis sizes (SMA: fast, slow; EMA: span, ols; BOLL: w,k,sl,tp)
    int32_t band_bps, k_den;
    int32_t wmax;                  // largest window of the grid (prefix ring sizing)
    int32_t ring;                  // prefix ring length >= wmax + 3 kTile (SMA: a power of two;
                                   // tile kernels: a multiple of kTile; plan.cpp plan_grid)
    double sqrt_ann;               // sqrt((double)annualization), computed on the host
    double kn2[8];                 // Bollinger: k_num^2 of the first 8 k values (kernel arguments,
                                   // so the z tests read them from scalar registers)
    int32_t kmin_idx;              // Bollinger: index of the smallest k_num (the busiest lanes)
    int32_t ablate;               // BT_PROFILING builds only (env BT_ABLATE): phases to skip;
                                   // always 0 in the release library (read through BT_ABL)
    const int32_t* a;              // device arrays
    const int32_t* b;
    const int32_t* c;
    const int32_t* d;
    // SMA key tasks (k_sma.hip stage_keys): the window lengths, fast rows then slow rows, padded
    // with length 1 to a whole kKeyGrab group, and their biased reciprocals key_recip(W). Read
    // with wave-uniform indices, so a group's values arrive in scalar registers.
    const int32_t* kwin;
    const double* krecip;
};
constexpr int kKeyGrab = 4;        // SMA windows per key task (one LDS atomic per group)

// Outputs of one run (device pointers).
struct Out {
    bt_summary* sum;               // [S * P]
    uint64_t* key;                 // [S * P] top-k order key (orderable sharpe)
    bt_sums* sums;                 // [S * P] parity mode, else nullptr
    bt_trade* trades;              // [S * P * trade_cap] parity mode, else nullptr
    int32_t trade_cap;
    unsigned long long* n_trades;  // total trades (one atomic per block)
    unsigned long long* dbg;       // profiling stamps (Grid::ablate & 64), else nullptr
};

// Bar-axis split of the tile kernels (k_ema.hip, k_boll.hip): each symbol's tiles are cut into G
// segments walked by separate workgroups. Segment s >= 1 starts flat `burn_tiles` tiles before
// its first bar (a walk whose accounting is discarded) and records the state it reached there;
// a fix pass per boundary re-walks a segment from the true state (the previous segment's end)
// if any lane's state differs, and a combine pass folds the segments' additive sums and
// max-plus drawdown forms into the summaries. One record per (segment, symbol, param), in
// result param order: rec[(s * n_sym + sym) * P + p].
struct SegRec {
    int32_t ntr, expo;
    int32_t start_pos, start_e;    // state at the segment's first accounted bar
    int32_t end_pos, end_e, end_ce, pad;
    int32_t end_agg[4];            // Agg of the open trade's path at the segment end
    int64_t R;                     // realized pnl of trades closed in the segment
    int64_t A, B, C, D;            // drawdown as functions of the entering gap g and mdd m:
                                   // gap' = max(g + A, B), mdd' = max(m, g + C, D)
    uint64_t h;                    // additive trade hash
    uint64_t s1lo;
    int64_t s1hi;
    uint64_t s2lo;
    int64_t s2hi;
};
static_assert(sizeof(SegRec) == 128, "SegRec layout");
// SMA bar segments (k_sma.hip): an SMA position is held from one crossover to the next, often
// for thousands of bars, so a segment cannot burn in to the entry of the trade open at its start.
// That trade is carried symbolically: the segment records where and at what price it closes
// and its path from the segment start, and the combine pass, which knows the entry from the
// earlier segments, closes it. One 128-B line per (segment, symbol, param), written whole by its
// lane (a full-line store; the combine reads it back once). The drawdown form A is -R (not
// stored) and the Sharpe sums' high words fit int32 (|S| < 2^78, spec §3).
struct SmaSegRec {
    int32_t ntr;                   // trades closed in the segment (the carried one included)
    int32_t e0;                    // first entry from flat in the segment (-1: none)
    int32_t start_pos, end_pos;    // position entering the first accounted bar / after the last
    int32_t end_e, end_ce;         // trade open at the end, opened in the segment (end_e = -1:
                                   // the carried trade is still open: entry unknown here)
    int32_t x1, px1;               // the carried trade's exit bar (-1: still open) and fill
    int32_t agg1[4];               // its path from the segment start to x1 (or to the end)
    int32_t end_agg[4];            // path of the trade open at the end, from its entry
    int64_t R;                     // pnl of the other trades closed in the segment (A = -R)
    int64_t B, C, D;               // their drawdown forms (SegRec)
    uint64_t h;                    // their additive hash
    uint64_t s1lo, s2lo;
    int32_t s1hi, s2hi;
};
static_assert(sizeof(SmaSegRec) == sizeof(SegRec), "SmaSegRec is one 128-B SegRec slot");
struct SegArgs {
    SegRec* rec;
    // SMA: the positions entering and leaving every (segment, symbol, param), int8 planes
    // [start | end] of G x S x P each: the fix pass compares them without touching the records
    int8_t* pos;
    unsigned long long* refixed;   // fix-pass blocks that re-walked their segment
    double* ema;                   // EMA+OLS: per (segment, symbol) the chains' values entering
                                   // the segment [0, 64) and leaving it [64, 128), lane = span
    int32_t G;                     // segments per symbol (1 = no split)
    int32_t burn_tiles;            // tiles walked before a speculative segment's first bar
};
constexpr int kEmaSegStride = 128;  // doubles per (segment, symbol) in SegArgs::ema
// Launchers (k_*.hip). All enqueue on `st` and return hipError_t. The strategy launchers enqueue
// what the run's LaunchPlan (plan.h) says: they decide nothing themselves.
struct LaunchPlan;
hipError_t launch_gen(const SymDesc* syms, int32_t n_sym, uint64_t seed, int32_t freq,
                      int32_t* o, int32_t* h, int32_t* l, int32_t* c, hipStream_t st);
hipError_t launch_sma(const SymDesc* syms, int32_t n_sym, const int32_t* close, const Grid& g,
                      const Out& out, bool parity, const SegArgs& seg, const LaunchPlan& pl,
                      hipStream_t st);
hipError_t launch_ema_ols(const SymDesc* syms, int32_t n_sym, const int32_t* close, const Grid& g,
                          const Out& out, bool parity, const SegArgs& seg, const LaunchPlan& pl,
                          hipStream_t st);
hipError_t launch_boll(const SymDesc* syms, int32_t n_sym, const int32_t* high, const int32_t* low,
                       const int32_t* close, const Grid& g, const Out& out, bool parity,
                       const SegArgs& seg, const LaunchPlan& pl, hipStream_t st);

// One (symbol, parameter) lane as the lane kernels (walk_tile.h LaneWalk) take it.
struct LaneRef {
    int64_t off;                   // SymDesc::off of the lane's symbol
    int32_t bars;
    int32_t param;
};

// The old name of LaneRef. Three stand-alone drivers (tests/plan/gram_plan_driver.cpp,
// tests/plan/replay_plan_driver.cpp, tests/asan/gram_driver.cpp) build with it, and 36 test cases
// build those drivers: it goes when a change may rewrite that many.
using ReplayLane = LaneRef;

// Replay of chosen lanes (k_replay.hip, bt_replay): one wave64 workgroup per request, which walks
// the symbol's rows and writes its summary, its first trade_cap trades and, when asked, E_t and
// pos_t of every bar. The buffers hold one chunk of requests; the host zeroes them before the
// launch (the kernel writes only trades that happen and bars that exist).
struct ReplayOut {
    bt_summary* sum;               // [n]
    bt_trade* trades;              // [n * trade_cap], or nullptr with trade_cap 0
    int32_t trade_cap;
    int64_t* equity;               // [n * pitch] or nullptr
    int8_t* pos;                   // [n * pitch] or nullptr
    int64_t pitch;                 // elements per curve row, >= the longest requested symbol
};
hipError_t launch_replay(const LaneRef* lanes, int32_t n, const int32_t* high, const int32_t* low,
                         const int32_t* close, const Grid& g, const ReplayOut& o, hipStream_t st);

// Walk-forward evaluation (k_walkfwd.hip, bt_walk_forward; docs/walkforward_spec.md) of one chunk
// of dataset rows. The walk (one wave64 workgroup per (row, param)) cuts every lane's path into K
// bar folds and leaves one bt_fold per (row, fold, param), params innermost so that the selection
// (one workgroup per (row, step)) reads along p. The host zeroes `rec` before the walk, which
// writes the records of non-empty folds and the first_bar of empty ones.
struct WfArgs {
    const SymDesc* syms;           // the chunk's rows
    const int32_t* bounds;         // [K + 1] fold bounds, absolute bars
    bt_fold* rec;                  // [n_rows][K][P]
    bt_wf_step* steps;             // [n_rows][n_steps] (selection only)
    int32_t n_rows, P, K;
    int32_t train, j0, n_steps;    // selection: steps j = j0 .. K - 1
};
struct WalkfwdPlan;
hipError_t launch_wf_walk(const WfArgs& a, const int32_t* high, const int32_t* low, const int32_t* close,
                          const Grid& g, hipStream_t st);
hipError_t launch_wf_select(const WfArgs& a, const Grid& g, const WalkfwdPlan& pl, hipStream_t st);

// Probability of backtest overfitting (k_cscv.hip, bt_cscv / bt_cscv_of; docs/cscv_spec.md) of one
// chunk of groups. The pack (one thread per (row, lane)) reads the s1/s2 words of the chunk's fold
// records, fold k of lane p of a row at rec[row * K * P + p * stride_p + k * stride_k], and leaves
// per lane K + 1 CscvSum (its folds, then their total) and per row its K return-bar counts. The
// combination kernel (one thread per combination pair, grid y = the launch's rows) adds to the
// group records and the histograms, which the host zeroes before a chunk's first launch, and
// stores the picks.
struct alignas(32) CscvSum {
    uint64_t s1_lo;
    int64_t s1_hi;
    uint64_t s2_lo;
    int64_t s2_hi;
};
struct CscvArgs {
    const bt_fold* rec;
    int64_t stride_p, stride_k;
    CscvSum* sums;                 // [n_rows][P][K + 1]
    int32_t* nret;                 // [n_rows][K]
    const uint32_t* masks;         // [pairs]
    bt_cscv_group* groups;         // [n_rows]
    uint32_t* hist;                // [n_rows][2P - 1] or nullptr
    bt_cscv_pick* picks;           // [n_rows][C] or nullptr
    int32_t n_rows, P, K;
    int64_t C, pairs;
};
struct CscvPlan;
hipError_t launch_cscv_pack(const CscvArgs& a, const CscvPlan& pl, hipStream_t st);
// rows [row0, row0 + rows) of the chunk, pairs [q0, q1) of each
hipError_t launch_cscv(const CscvArgs& a, const CscvPlan& pl, int32_t row0, int32_t rows, int64_t q0, int64_t q1,
                       double sqrt_ann, hipStream_t st);

// Trade statistics (k_tstats.hip, bt_trade_stats; docs/tradestats_spec.md) of one chunk. The walk
// (one wave64 workgroup per lane) leaves one bt_tstats per lane: with `lanes` the n staged
// requests in order, else lane row * P + param of the chunk's n_rows dataset rows. The reduction
// adds a chunk's [n_rows][P] records into agg[P], which the host zeroes before the first chunk.
struct TsArgs {
    const SymDesc* syms;           // the chunk's rows (all-lanes mode)
    const LaneRef* lanes;          // the chunk's requests (list mode), else nullptr
    bt_tstats* rec;                // [n] or [n_rows][P]
    bt_tstats_agg* agg;            // [P] (reduction only)
    int32_t n, n_rows, P;
};
struct TstatsPlan;
hipError_t launch_tstats_walk(const TsArgs& a, const int32_t* high, const int32_t* low, const int32_t* close,
                              const Grid& g, hipStream_t st);
hipError_t launch_tstats_agg(const TsArgs& a, const TstatsPlan& pl, hipStream_t st);

// Net of costs (k_costs.hip, bt_costs; docs/costs_spec.md) of one chunk. The walk (one wave64
// workgroup per lane) leaves C bt_cost_rec per lane, levels innermost: with `lanes` the n staged
// requests in order, else lane row * P + param of the chunk's n_rows dataset rows. The reduction
// adds a chunk's [n_rows][P][C] records into agg[P][C], which the host zeroes before the first
// chunk. The level table travels by value beside the arguments: one address for the whole grid,
// read by scalar loads.
struct CostArgs {
    const SymDesc* syms;           // the chunk's rows (all-lanes mode)
    const LaneRef* lanes;          // the chunk's requests (list mode), else nullptr
    bt_cost_rec* rec;              // [n][C] or [n_rows][P][C]
    bt_cost_agg* agg;              // [P][C] (reduction only)
    int32_t n, n_rows, P, C;
};
struct CostLevels {
    int32_t fixed[BT_COST_LEVELS_MAX], bps[BT_COST_LEVELS_MAX];
};
struct CostsPlan;
hipError_t launch_cost_walk(const CostArgs& a, const CostLevels& lv, const int32_t* high, const int32_t* low,
                            const int32_t* close, const Grid& g, hipStream_t st);
hipError_t launch_cost_agg(const CostArgs& a, const CostsPlan& pl, hipStream_t st);

// Tail risk (k_tail.hip, bt_tail / bt_tail_of; docs/tail_spec.md) of one chunk of m lanes, one
// workgroup each: with `lanes` the chunk's staged requests, with `d` its staged rows of T increments
// ([m][pitch]), else lane row * P + param of the chunk's dataset rows. rec and q may each be nullptr.
struct TailArgs {
    const SymDesc* syms;           // the chunk's rows (all-lanes mode)
    const LaneRef* lanes;          // the chunk's requests (list mode), else nullptr
    const int32_t* levels;         // [Q] alpha_ppm
    bt_tail_rec* rec;              // [m] or nullptr
    bt_tail_q* q;                  // [m][Q] or nullptr
    int32_t* rows;                 // [m][pitch]: the arena rows, or the staged increments
    int64_t pitch;
    int32_t P, Q, from, to, held;  // the window [from, to) (to already resolved), BT_TAIL_HELD
    int32_t T;                     // bars of a staged row
    int32_t cap;                   // counted bars a lane's row holds (the plan's longest_n)
};
struct TailPlan;
hipError_t launch_tail_walk(const TailArgs& a, int32_t m, const TailPlan& pl, const int32_t* high, const int32_t* low,
                            const int32_t* close, const Grid& g, hipStream_t st);
hipError_t launch_tail_of(const TailArgs& a, int32_t m, const TailPlan& pl, hipStream_t st);

// Bootstrap reality check (k_boot.hip, bt_bootstrap / bt_bootstrap_of; docs/bootstrap_spec.md).
// The start kernel fills the start table and sets vmax to INT64_MIN once per call; the lane kernel
// (one workgroup per lane of a chunk: lane lane0 + blockIdx.x of the call) builds the lane's prefix
// row, by a LaneWalk or from staged increments, resamples it and leaves the lane's record, its row
// of boot and its part of vmax; the finish (one workgroup per group) leaves the group records.
struct BootArgs {
    const SymDesc* syms;           // all-lanes mode: the dataset's rows, lane = row * P + param
    const LaneRef* lanes;          // [n] with a lane list, else nullptr
    const int32_t* gid;            // [n] every lane's group, or nullptr: lane / P
    const int32_t* d;              // staged: the chunk's increments [m][d_pitch]
    const int32_t* starts;         // [K][B]
    int64_t* rows;                 // the chunk's prefix rows [m][pitch] (arena path), else nullptr
    int64_t* vmax;                 // [G][B]
    int64_t* boot;                 // [n][B] or nullptr
    bt_boot_lane* rec;             // [n]
    const int32_t* goff;           // [G + 1], or nullptr: g * P
    bt_boot_group* groups;         // [G]
    int64_t lane0;                 // the chunk's first lane
    int64_t pitch, d_pitch;
    int32_t P, G;
    int32_t from, T, B, Lp, K, last_len;
};
struct BootPlan;
hipError_t launch_boot_starts(const BootArgs& a, const BootPlan& pl, uint64_t seed, hipStream_t st);
hipError_t launch_boot_walk(const BootArgs& a, int32_t m, const BootPlan& pl, const int32_t* high, const int32_t* low,
                            const int32_t* close, const Grid& g, hipStream_t st);
hipError_t launch_boot_prefix(const BootArgs& a, int32_t m, const BootPlan& pl, hipStream_t st);
hipError_t launch_boot_finish(const BootArgs& a, const BootPlan& pl, hipStream_t st);

// Drawdown bootstrap (k_ddboot.hip, bt_drawdown_boot / bt_drawdown_boot_of; docs/drawdown_spec.md)
// of one chunk of m lanes, one workgroup each, over the start table launch_boot_starts made: with
// `lanes` the chunk's staged requests, with `d` its staged rows of increments, else lane lane0 +
// blockIdx.x of the dataset, row * P + param. Every output is the chunk's own and may be nullptr.
struct DdArgs {
    const SymDesc* syms;           // all-lanes mode: the dataset's rows
    const LaneRef* lanes;          // [m] the chunk's requests (list mode), else nullptr
    const int32_t* d;              // [m][d_pitch] staged increments, else nullptr
    const int32_t* starts;         // [K][B]
    const int32_t* levels;         // [Q] alpha_ppm
    const int64_t* limits;         // [R]
    unsigned char* rows;           // [m][pitch] bytes: the arena rows (prefix row, then the tables), else nullptr
    int64_t* vals;                 // [m][v_pitch]: the values of the selection when they are neither in LDS nor in raw
    int64_t* raw;                  // [m][B] or nullptr
    bt_dd_lane* rec;               // [m] or nullptr
    int64_t* q;                    // [m][Q] or nullptr
    int64_t* reach;                // [m][R] or nullptr
    int64_t lane0;                 // the chunk's first lane (all-lanes mode)
    int64_t pitch, d_pitch, v_pitch;
    uint32_t r_w1, r_w2;           // bytes from the row's start to the two tables (equal: one table)
    uint32_t l_vals;               // bytes from the start of LDS to the values of the selection (0: not in LDS)
    int32_t P;
    int32_t from, T, B, Lp, K, last_len, Q, R;
};
struct DdPlan;
// Once a call, before its chunks: asks for the dynamic LDS of the call's kernel where it passes 64 KB.
hipError_t prepare_dd(const DdPlan& pl, bool staged, const Grid& g);
hipError_t launch_dd_walk(const DdArgs& a, int32_t m, const DdPlan& pl, const int32_t* high, const int32_t* low,
                          const int32_t* close, const Grid& g, hipStream_t st);
hipError_t launch_dd_of(const DdArgs& a, int32_t m, const DdPlan& pl, hipStream_t st);

// Portfolio of chosen lanes (k_portfolio.hip, bt_portfolio; docs/portfolio_spec.md). The walk (one
// wave64 workgroup per entry) adds every entry's per-bar pnl and position into replicated per-bar
// accumulators with integer atomics; the finish (one block) folds the replicas into the output
// rows, scans the equity and writes the summary. The host passes only entries whose clipped
// window [from, to) is not empty, to <= min(bars, T), and zeroes the accumulators before the walk.
struct PfLane : LaneRef {
    int32_t from, to;              // the clipped window
};
static_assert(sizeof(PfLane) == 24, "PfLane layout");
struct PfWork {
    unsigned long long* acc_pnl;   // [R][pitch] sums of E_t - E_(t-1)
    unsigned long long* acc_cnt;   // [R][pitch] n_long | n_short << 32
    int64_t pitch;                 // elements per accumulator row: T rounded up to a tile
    int32_t R;                     // replicas: workgroup b adds to replica b % R
    int32_t T;                     // bars of the output rows
    int32_t n_lanes, lo, hi;       // of the summary: entries, first bar, one past the last bar
    int64_t* pnl;                  // [T] outputs
    int64_t* equity;
    int32_t* n_long;
    int32_t* n_short;
    bt_pf_summary* sum;
};
struct PortfolioPlan;
hipError_t launch_portfolio(const PfLane* lanes, int32_t n, const int32_t* high, const int32_t* low,
                            const int32_t* close, const Grid& g, const PfWork& w, const PortfolioPlan& pl,
                            hipStream_t st);

// Covariance of chosen lanes (k_gram.hip, bt_covariance / bt_gram_of; docs/covariance_spec.md).
// The walk (one wave64 workgroup per lane) writes the lane's increments over the window into row i
// of the int32 matrix D and its row sum; the product (one wave per 16 x 16 tile with I <= J and
// bar chunk) forms D * D^T on the fp64 matrix cores and leaves one exact int128 per element and
// chunk; the fold adds the chunks, mirrors the upper triangle and writes gram[n][n] (and the row
// sums of a staged D). The host zeroes D before the walk or the upload: its padding is zero.
struct GramWork {
    int32_t* D;                    // [n][pitch] increments, column t - from_bar
    int64_t pitch;                 // elements per row: T rounded up to 64
    bt_wide* partial;              // [chunks][tiles][256], tile (I, J) of I <= J at I*nt - I*(I-1)/2 + J - I
    bt_wide* gram;                 // [n][n]
    int64_t* sums;                 // [n]
    int32_t n, T;
    int32_t nt;                    // 16-row tiles along n
    int32_t tiles;                 // nt * (nt + 1) / 2
    int32_t chunks, chunk_bars;    // bar chunks and the bars of one (a multiple of 64)
};
struct GramPlan;
hipError_t launch_gram_walk(const LaneRef* lanes, const int32_t* high, const int32_t* low,
                            const int32_t* close, const Grid& g, const GramWork& w, int32_t from, int32_t to,
                            hipStream_t st);
// `staged`: D was uploaded (bt_gram_of) and the fold writes the row sums too.
hipError_t launch_gram(const GramWork& w, const GramPlan& pl, bool staged, hipStream_t st);

// Reductions of an S x P summary matrix (k_surface.hip, bt_surface / bt_surface_of): one pass over
// the records writes per-chunk column aggregates and per-tile row winners, two short kernels fold
// them into agg[P] and best[S]. Symbol s has id ids[s * id_stride] (the engine's SymDesc array or
// a plain id list). Either output may be nullptr; the shape is the SurfacePlan's (plan.h).
struct SurfacePlan;
struct SurfaceWork {
    bt_param_agg* partial;         // [chunks * P]
    bt_param_agg* fold;            // [fold_ways * P]: the first fold step's output
    bt_topk_rec* best_partial;     // [S * p_tiles]
    bt_param_agg* agg;             // [P] or nullptr
    bt_topk_rec* best;             // [S] or nullptr
};
hipError_t launch_surface(const bt_summary* sum, const int32_t* ids, int32_t id_stride, int32_t S,
                          int32_t P, const SurfacePlan& pl, const SurfaceWork& w, hipStream_t st);

// Top-k by radix select over `key` (k_topk.hip): device-side finish into `out`.
constexpr int kTopkCap = 2048;      // candidates sorted in LDS by the finish kernel
constexpr int kTopkMax = 1024;      // largest k the engine accepts
struct TopkWork {
    unsigned int* hist;            // [4096]
    unsigned long long* state;     // [4]: prefix, decided-bit mask, remaining need
    unsigned int* counts;          // [2]: above, candidates
    unsigned long long* above;     // [cap]
    unsigned long long* cand;      // [cap]
    int cap;
    bt_topk_rec* out;              // [k]
    int32_t* out_n;                // [1]: records written, -1 = overflow (host finishes)
};
hipError_t launch_topk(const uint64_t* key, const bt_summary* sum, const SymDesc* syms,
                       int64_t n, int32_t P, int32_t k, const TopkWork& w, hipStream_t st, bool lds_free_hist = false);
hipError_t launch_topk_init(const TopkWork& w, hipStream_t st);  // once per buffer allocation

// Host-side pieces shared by engine.cpp and comm.cpp.
inline bool topk_less(const bt_topk_rec& a, const bt_topk_rec& b);  // "a ranks before b"
struct ExchangeView {
    hipStream_t tstream;
    int32_t device, topk;
    const bt_topk_rec* d_top;            // [0] = header (record count), then topk records
    const unsigned long long* d_ntr;     // trades of the last run
    int64_t bar_evals;
};
bool engine_exchange_view(bt_engine* e, ExchangeView& v, std::string& err);
void engine_exchange_enqueued(bt_engine* e);

// Shared host/device helpers.
// Upward-biased reciprocal for exact floor keys (k_sma.hip floor_key): RN(RN(1/W) * (1 + 2^-47)),
// two correctly rounded IEEE operations on the host as on the device.
__host__ __device__ inline double key_recip(int W) { return (1.0 / (double)W) * (1.0 + 0x1p-47); }

__host__ __device__ inline uint64_t order_key(double x) {
    union { double d; uint64_t u; } v;
    v.d = x;
    return (v.u >> 63) ? ~v.u : (v.u | 0x8000000000000000ULL);
}

// int128 (lo, hi) -> double, round to nearest, ties to even (spec §4 conversion).
__host__ __device__ inline double i128_to_double(uint64_t lo, int64_t hi) {
    const bool neg = hi < 0;
    uint64_t mh = (uint64_t)hi, ml = lo;
    if (neg) {  // two's complement negate
        ml = ~ml + 1;
        mh = ~mh + (ml == 0 ? 1 : 0);
    }
    if (mh == 0 && ml == 0) return 0.0;
    int lz = mh ? __builtin_clzll(mh) : 64 + __builtin_clzll(ml);
    // normalise: leading one to bit 127
    uint64_t nh, nl;
    if (lz >= 64) {
        nh = ml << (lz - 64);
        nl = 0;
    } else if (lz == 0) {
        nh = mh;
        nl = ml;
    } else {
        nh = (mh << lz) | (ml >> (64 - lz));
        nl = ml << lz;
    }
    // top 53 bits = nh >> 11; remainder = low 11 bits of nh and all of nl
    uint64_t mant = nh >> 11;
    const uint64_t rem_hi = nh & 0x7FFULL;  // 11 bits
    const uint64_t half = 0x400ULL;
    bool up;
    if (rem_hi > half) up = true;
    else if (rem_hi < half) up = false;
    else up = (nl != 0) || (mant & 1);
    mant += up ? 1 : 0;
    // value = mant * 2^(127 - lz - 52)
    double r = (double)mant;  // exact: mant <= 2^53
#ifdef __HIP_DEVICE_COMPILE__
    r = ldexp(r, 75 - lz);
#else
    r = __builtin_ldexp(r, 75 - lz);
#endif
    return neg ? -r : r;
}

// The order of bt_topk_rec on the host (bt_merge_topk, comm.cpp merge_block). Ids compare as int32
// here and as unsigned words on the device (k_topk.hip sym_param): one order, because every symbol
// id lies in [0, 2^31) (topk_rules.h).
inline bool topk_less(const bt_topk_rec& a, const bt_topk_rec& b) {
    const uint64_t ka = order_key(a.sharpe), kb = order_key(b.sharpe);
    if (ka != kb) return ka > kb;
    if (a.sym != b.sym) return a.sym < b.sym;
    return a.param < b.param;
}

__host__ __device__ inline double sharpe_fx(uint64_t s1lo, int64_t s1hi, uint64_t s2lo,
                                            int64_t s2hi, int32_t bars, double sqrt_ann) {
    if (bars < 2) return 0.0;
    const double n = (double)(bars - 1);
    const double m = ldexp(i128_to_double(s1lo, s1hi), -56) / n;
    const double mm = m * m;
    const double v = ldexp(i128_to_double(s2lo, s2hi), -56) / n - mm;
    return v > 0 ? (m / sqrt(v)) * sqrt_ann : 0.0;
}
__host__ __device__ inline double sharpe_fx(i128 s1, i128 s2, int32_t bars, double sqrt_ann) {
    return sharpe_fx(wide_lo(s1), wide_hi(s1), wide_lo(s2), wide_hi(s2), bars, sqrt_ann);
}

// Sharpe of a portfolio's per-bar tick increments (docs/portfolio_spec.md §4): the oracle's
// formula on s1 = sum pnl[t], s2 = sum pnl[t]^2 over the n bars [lo, hi); 0 when there is none.
__host__ __device__ inline double sharpe_ticks(uint64_t s1lo, int64_t s1hi, uint64_t s2lo,
                                               int64_t s2hi, int32_t n_bars, double sqrt_ann) {
    if (n_bars < 1) return 0.0;
    const double n = (double)n_bars;
    const double m = i128_to_double(s1lo, s1hi) / n;
    const double mm = m * m;
    const double v = i128_to_double(s2lo, s2hi) / n - mm;
    return v > 0 ? (m / sqrt(v)) * sqrt_ann : 0.0;
}
__host__ __device__ inline double sharpe_ticks(i128 s1, i128 s2, int32_t n_bars, double sqrt_ann) {
    return sharpe_ticks(wide_lo(s1), wide_hi(s1), wide_lo(s2), wide_hi(s2), n_bars, sqrt_ann);
}

}  // namespace bt
