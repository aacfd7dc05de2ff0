/*
 * bt.h — C ABI of the MI355X-native backtest engine (libbt.so).
 *
 * This is the drop-in boundary for the reference worker's job function
 *     pub fn process_incoming_job(jobs_reply: JobsReply, complete_send: Sender<String>)
 *     (/root/reference/src/worker/process.rs:13-29)
 * which today sleeps 1000 ms per job (process.rs:23) and sends `job.id` per job (process.rs:24),
 * called from the worker's single compute OS thread (/root/reference/src/worker/main.rs:38-42).
 * The proto contract stays byte-identical (/root/reference/proto/backtesting.proto):
 * `Job{string id; bytes File}` in (proto:13-16), `CompleteRequest{string id; string data}` out
 * (proto:29-32). The Rust-side `extern "C"` block a maintainer would add is in INTEGRATION.md.
 *
 * Plain C types only. No C++ exception and no abort crosses this boundary: every entry point
 * catches and returns an int status (0 = OK, < 0 = error; message via bt_last_error()).
 * The engine is not thread-safe (the reference has exactly one caller thread, main.rs:38-42);
 * it sets its HIP device on every call, so it may be called from any one OS thread.
 * Semantics of every number produced: docs/oracle_spec.md.
 */
#ifndef BT_H
#define BT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: bt_batch_profile.payload_bytes_read; the device top-k never overflows (bt_topk_fetch_wait
 *    and bt_exchange_wait return exact records on tie-heavy grids); bt_summary.hash is the
 *    additive trade hash of docs/oracle_spec.md §4 (version 1 hosts may hold FNV-1a hashes).
 * 3: bt_exchange_merge takes the gathered block's byte length and rejects a mismatch. */
#define BT_ABI_VERSION 3

typedef struct bt_engine bt_engine;

enum bt_strategy { BT_SMA_CROSS = 1, BT_EMA_OLS = 2, BT_BOLL = 3 };

enum bt_flags {
    BT_FLAG_PARITY = 1,  /* also record full trade lists and the int128 return sums */
    BT_FLAG_TIMING = 2,  /* time the dominant kernel with HIP events (bt_kernel_timing) */
};

enum bt_freq { BT_DAILY = 0, BT_MINUTE = 1 };

/* Engine configuration. The proto carries no strategy or params (proto:13-16), so the grid is
 * worker-side configuration (SURVEY.md §7 hard part 5). Arrays are copied at create time.
 * Accepted domain (docs/oracle_spec.md §7): windows up to 4,096 bars always, longer ones while the
 * prefix ring fits 160 KB of LDS; EMA at most 64 spans; Bollinger w * max(k_num, k_den) < 2^32;
 * at most 2^20 params. Anything else is refused by bt_engine_create, never approximated. */
typedef struct bt_config {
    int32_t strategy;                 /* enum bt_strategy */
    /* SMA crossover: params = n_fast x n_slow, param = i_fast * n_slow + i_slow */
    int32_t n_fast, n_slow;
    const int32_t* fast;
    const int32_t* slow;
    /* EMA + rolling OLS: params = n_span x n_ols, param = i_span * n_ols + i_ols */
    int32_t n_span, n_ols;
    const int32_t* span;
    const int32_t* ols;
    int32_t band_bps;
    /* Bollinger + SL/TP: param = ((i_w * n_k + i_k) * n_sl + i_sl) * n_tp + i_tp */
    int32_t n_bwin, n_k, n_sl, n_tp;
    const int32_t* bwin;
    const int32_t* k_num;
    int32_t k_den;
    const int32_t* sl_bps;
    const int32_t* tp_bps;
    int64_t annualization;            /* A in the Sharpe formula: 252 daily, 98280 1-min */
    int32_t device;                   /* HIP device ordinal */
    int32_t topk;                     /* k of bt_read_topk (0 = top-k disabled) */
    int32_t flags;                    /* enum bt_flags */
    int32_t host_threads;             /* CSV parse threads in bt_run_batch (0 = auto) */
    int32_t trade_cap;                /* parity mode: trades kept per (symbol, param) */
    void* stream;                     /* optional hipStream_t to launch on (NULL = own stream) */
} bt_config;

/* One Job of a JobsReply (proto:13-16). Borrowed for the duration of the call. */
typedef struct bt_job_in {
    const char* id;                   /* Job.id (UUIDv4 string from server/main.rs:169) */
    const uint8_t* file;              /* Job.File bytes (whole CSV, server/main.rs:170) */
    size_t len;
} bt_job_in;

/* One CompleteRequest.data (proto:31, UTF-8). Owned by the library: free with bt_job_out_free. */
typedef struct bt_job_out {
    char* data;
    size_t len;
    int32_t status;                   /* 0 = OK, < 0 = this job failed (data holds {"error":..}) */
    int32_t n_bars;
} bt_job_out;

/* Per (symbol, param) result, 48 bytes. */
typedef struct bt_summary {
    int32_t n_trades;
    int32_t status;
    int64_t pnl;                      /* ticks */
    int64_t mdd;                      /* ticks */
    int64_t exposure;                 /* bars held */
    double sharpe;
    uint64_t hash;                    /* additive trade-sequence hash (spec §4) */
} bt_summary;

typedef struct bt_trade {
    int32_t entry_bar, exit_bar, side, pad;
    int64_t entry_px, exit_px;
} bt_trade;

/* S1, S2 of spec §4 (int128 as lo/hi words); parity mode only. */
typedef struct bt_sums {
    uint64_t s1_lo;
    int64_t s1_hi;
    uint64_t s2_lo;
    int64_t s2_hi;
} bt_sums;

/* Global top-k record (24 B): ordered by sharpe desc, then sym asc, then param asc. Sharpe by its
 * orderable bit pattern (+0.0 ranks above -0.0). sym is a symbol id, and symbol ids lie in
 * [0, 2^31): there the device's unsigned tie-break and the host's signed compare are one order. */
typedef struct bt_topk_rec {
    double sharpe;
    int32_t sym;
    int32_t param;
    int64_t pnl;
} bt_topk_rec;

typedef struct bt_stats {
    int64_t n_symbols;
    int64_t n_params;
    int64_t bar_evals;                /* sum over symbols of bars x params */
    int64_t trades;                   /* sum of n_trades over every (symbol, param) */
    int64_t errors;                   /* symbols rejected */
} bt_stats;

/* ---- lifecycle */
bt_engine* bt_engine_create(const bt_config* cfg, char* err, size_t errlen);
void bt_engine_destroy(bt_engine* e);
const char* bt_last_error(void);      /* thread-local message of the last failed call */
int32_t bt_abi_version(void);
int32_t bt_num_params(const bt_engine* e);
/* Bar-axis split of every strategy's walk (k_ema.hip, k_boll.hip, k_sma.hip): segments per symbol (0 =
 * automatic: EMA+OLS and Bollinger split a shard with no more workgroups than the GPU has CUs, SMA
 * a shard of one-block-per-CU symbols that fills the GPU fewer than 16 times; 1 = never; n =
 * always n) and the burn-in tiles a speculative segment walks before its first bar (0 = the
 * default: 64 for Bollinger, 24 x the longest span for EMA+OLS, so every fp64 EMA chain meets the
 * true one, 2 for SMA, whose trade open at a boundary is carried symbolically into a combine
 * pass). Results are identical either way (a boundary whose speculative start differs from
 * the true one is re-walked); parity mode (trade lists) never splits. bt_last_segments: the count
 * the last bt_run used and, if refixed_blocks is not NULL, how many (symbol, boundary) blocks the
 * fix pass re-walked (waits for the run). */
int32_t bt_set_segments(bt_engine* e, int32_t segments, int32_t burn_tiles);
int32_t bt_last_segments(bt_engine* e, int64_t* refixed_blocks);

/* Consecutive bt_run calls of an engine that owns its stream go to two streams in turn, so that a
 * run's first blocks take the compute units the run before it frees as it drains (on: the
 * default). A run that is split into bar segments, a parity-mode run, a run whose blocks all fit
 * on the device at once (nothing queues behind it) and every run of an engine on a caller's stream
 * (bt_config.stream) never overlap another run, whatever is set here: there the call succeeds and
 * the engine stays serial. Results are identical either way, and every
 * other call is ordered behind all earlier runs as before: the records of run i are valid after
 * its fetch. 0 = off: every run waits for the one before it. */
int32_t bt_set_run_overlap(bt_engine* e, int32_t on);

/* Phase times of the last bt_run_batch call (host clocks for host phases, HIP events for the
 * device ones). */
typedef struct bt_batch_profile {
    int64_t n_jobs, n_failed;
    int64_t payload_bytes;            /* sum of Job.File lengths */
    int64_t payload_bytes_read;       /* bytes ingest actually reads: a CSV whole, a DBXCOL1
                                         payload its header and price columns (never the
                                         volume column) */
    int64_t bars;                     /* bars of the good jobs */
    double host_ingest_ms;            /* parse / validate + copy into pinned staging */
    double upload_ms;                 /* H2D of the staged columns */
    double compute_ms;                /* strategy kernel (+ top-k when enabled) */
    double readback_ms;               /* one D2H of every summary of the batch */
    double format_ms;                 /* CompleteRequest.data strings */
    double total_ms;                  /* wall time of the call */
} bt_batch_profile;

/* ---- drop-in for process_incoming_job: a whole JobsReply in one GPU launch.
 * outs[i] answers jobs[i] (same order the reference sends completions, process.rs:21-25).
 * On a -1 return no output string is left allocated (outs are all NULL). */
int32_t bt_run_batch(bt_engine* e, size_t n, const bt_job_in* jobs, bt_job_out* outs);
void bt_job_out_free(bt_job_out* outs, size_t n);
int32_t bt_last_batch_profile(bt_engine* e, bt_batch_profile* out);

/* ---- HBM-resident path (configs 2-5, bench, multi-GPU shards) */
/* Generate n_sym synthetic symbols (spec §1) with ids sym_begin.. directly in HBM. */
int32_t bt_load_synthetic(bt_engine* e, uint64_t seed, int64_t sym_begin, int32_t n_sym,
                          int32_t n_bars, int32_t freq);
/* Upload host SoA bars: symbol s has bars[s] rows starting at row offset row_off[s] in h/l/c.
 * h and l may be NULL unless the strategy is BT_BOLL. Every sym_ids[s] must lie in [0, 2^31) (the
 * range bt_load_synthetic generates; the engine keeps ids as int32 and orders ties by them): an id
 * outside it is refused with its index and value named, before anything is laid out, so the
 * dataset loaded before stays resident and the engine usable. */
int32_t bt_load_ohlc(bt_engine* e, int32_t n_sym, const int64_t* sym_ids, const int32_t* bars,
                     const int64_t* row_off, const int32_t* h, const int32_t* l,
                     const int32_t* c);
int32_t bt_run(bt_engine* e);         /* enqueue the whole hot path on the engine stream */
int32_t bt_sync(bt_engine* e);
int32_t bt_read_summaries(bt_engine* e, bt_summary* out, size_t n);     /* n = symbols x params */
int32_t bt_read_sums(bt_engine* e, bt_sums* out, size_t n);             /* parity mode */
int32_t bt_read_trades(bt_engine* e, bt_trade* out, size_t n);          /* n = sym x param x cap */
int32_t bt_read_topk(bt_engine* e, bt_topk_rec* out, int32_t k);        /* returns count */
int32_t bt_read_stats(bt_engine* e, bt_stats* out);
#define BT_PIPE_SLOTS 4 /* pinned read-back / exchange slots per engine / communicator */
/* Pipelined read-back of the last run's top-k and trade count: bt_topk_fetch_async enqueues
 * the device-to-host copy into pinned slot 0 .. BT_PIPE_SLOTS-1 behind the run (no host wait),
 * so the next bt_run (or the next BT_PIPE_SLOTS - 1) can be enqueued before this run's records
 * are consumed; bt_topk_fetch_wait waits for
 * that copy only and returns the record count. The device selection is exact on any grid (a
 * tie-heavy one takes a slower single-block finish, k_topk.hip). A slot stays valid until its
 * next fetch. */
int32_t bt_topk_fetch_async(bt_engine* e, int32_t slot);
int32_t bt_topk_fetch_wait(bt_engine* e, int32_t slot, bt_topk_rec* out, int32_t k,
                           int64_t* n_trades);
/* Read back the synthetic/uploaded close column of one symbol (tests). */
int32_t bt_read_close(bt_engine* e, int32_t sym_index, int32_t* out, int32_t n);
/* ---- replay of chosen lanes: trades, position and equity curve (k_replay.hip)
 * Runs n (symbol, param) lanes of the dataset the engine holds (whatever the last
 * bt_load_synthetic, bt_load_ohlc or bt_run_batch left resident; bt_run need not have been
 * called) again, one wave per lane, and returns per lane, in request order (repeats allowed):
 *   sum[i]      the full bt_summary, every field as bt_run produces it;
 *   n_bars[i]   the bars of lane i's symbol;
 *   trades      row i (trade_cap records): the first min(n_trades, trade_cap) trades, then zeros;
 *   equity      row i (stride values): E_t of spec §4 at the close of every bar, then zeros;
 *   pos         row i (stride values): pos_t after bar t (-1, 0, +1), then zeros.
 * bt_lane.sym is the global symbol id of bt_topk_rec.sym, so top-k records feed straight in; with
 * duplicate ids in the dataset the first row wins. Added within ABI 3 (additive).
 * Synchronous: waits for the engine's streams, runs on the engine stream, copies back, returns n
 * (0 for n == 0). It changes nothing an existing entry point reads: summaries, top-k, stats,
 * timing counters, segments, pipeline slots and the run state are as before the call.
 * Device staging is bounded: the lanes are processed in chunks against a fixed 256 MB budget,
 * never n * stride, and freed by bt_engine_destroy. Any grid bt_engine_create accepts replays (the
 * kernel keeps no window-sized state). Returns -1, with bt_last_error naming the offending value,
 * for: a null engine, no dataset, n < 0 or n > BT_REPLAY_MAX, an unknown symbol id, param outside
 * [0, P), trade_cap < 0, trades given with trade_cap 0 or the reverse, stride shorter than the
 * longest requested symbol when equity or pos is given. The engine stays usable after a refusal. */
typedef struct bt_lane {
    int32_t sym;                      /* global symbol id (bt_topk_rec.sym) */
    int32_t param;
} bt_lane;
#define BT_REPLAY_MAX 4096            /* lanes per call */
int32_t bt_replay(bt_engine* e, int32_t n, const bt_lane* lanes, int32_t trade_cap,
                  bt_summary* sum,    /* [n], required */
                  int32_t* n_bars,    /* [n] or NULL */
                  bt_trade* trades,   /* [n * trade_cap] or NULL (then trade_cap must be 0) */
                  int64_t* equity,    /* [n * stride] or NULL */
                  int8_t* pos,        /* [n * stride] or NULL */
                  int64_t stride);    /* >= the longest requested symbol when equity or pos is given */
/* ---- reductions of a run (k_surface.hip, surface.cpp; semantics: docs/surface_spec.md)
 * The S x P summaries a run leaves in HBM, reduced along each axis on the device:
 *   agg[p]   one bt_param_agg per parameter over every row with status == 0 (the "parameter
 *            surface"): counts, int64 sums, the worst drawdown, the fixed-point Sharpe sums
 *            ss1 = sum qs, ss2 = sum qs^2 (int128 as lo/hi words like bt_sums,
 *            qs = rint(clamp(sharpe, +-2^15) * 2^32)), and the best and worst symbol;
 *   best[s]  one bt_topk_rec per dataset row, in row order: the row's first lane in the top-k
 *            order (Sharpe descending, then param ascending), sym = the global id. Feeds bt_replay.
 * Every field is order-independent: any chunking and any split over ranks gives the same bits.
 * Added within ABI 3 (additive). */
typedef struct bt_param_agg {           /* 104 bytes */
    int32_t n_sym, n_traded, n_win, n_pos;   /* rows counted; with n_trades > 0, pnl > 0, sharpe > 0 */
    int64_t trades, pnl, exposure, mdd_max;  /* sums; the largest mdd (0 when n_sym == 0) */
    double  sharpe_max, sharpe_min;          /* 0.0 when n_sym == 0 */
    int32_t sym_max, sym_min;                /* their symbols' ids, ties to the lowest; -1 when n_sym == 0 */
    uint64_t ss1_lo; int64_t ss1_hi; uint64_t ss2_lo; int64_t ss2_hi;
} bt_param_agg;

/* Reduce the last run's summaries on the device. agg[P] and/or best[S] (either may be NULL, not
 * both). Synchronous like bt_replay: waits for the engine's streams, runs on the engine stream,
 * copies back; changes nothing another entry point reads. Works after bt_run and bt_run_batch.
 * Returns 0, or -1 with bt_last_error naming the offending value (the engine stays usable): a null
 * engine, no run yet, both outputs NULL, a dataset of 2^32 rows or more (the int64 sums are exact
 * only below that and are never wrapped). */
int32_t bt_surface(bt_engine* e, bt_param_agg* agg, bt_topk_rec* best);
/* The same device kernels on a caller's matrix (row-major S x P, sym_ids[S]); S*P <= 2^22. S == 0
 * gives P empty aggregates and no best record; S < 0 or P < 1 is refused. */
int32_t bt_surface_of(bt_engine* e, int32_t S, int32_t P, const bt_summary* sum,
                      const int32_t* sym_ids, bt_param_agg* agg, bt_topk_rec* best);
/* The run's top-k chain (k_topk.hip: radix select, then the sort or the tie finish in one block)
 * on a caller's records: sum is a row-major S x P matrix, sym_ids[S] the rows' ids, and out[k]
 * receives the min(k, S*P) best records in the order of bt_topk_rec, exactly what bt_read_topk
 * would return after a run that left these summaries. lds_free_hist != 0 selects the histogram
 * kernel without LDS (used up to 2^18 records, as in a run). Returns the number of records
 * written. Synchronous like bt_replay: waits for the engine's streams, runs on the engine stream,
 * copies back. Its whole work set is staged beside the records, so it works on any engine (also
 * one created with topk = 0 and no dataset) and changes nothing another entry point reads. Added
 * within ABI 3 (additive). Returns -1 with bt_last_error naming the offending value (the engine
 * stays usable): a null engine, S < 1 or P < 1, S*P > 2^22, k outside [1, 1024], a NULL sum,
 * sym_ids or out, an id below 0. */
int32_t bt_topk_of(bt_engine* e, int32_t S, int32_t P, const bt_summary* sum,
                   const int32_t* sym_ids, int32_t k, int32_t lds_free_hist, bt_topk_rec* out);
/* Symbol chunks the reduction is cut into: 0 = the planner's choice, n = always n (clipped to S).
 * Results are identical either way. */
int32_t bt_set_surface_chunks(bt_engine* e, int32_t chunks);
/* Host, no GPU needed: the scalar restatement, and the merge of `world` aggregates of P records
 * (in[w * P + p], disjoint symbol sets; world >= 1) into out[P]. */
int32_t bt_surface_host(int32_t S, int32_t P, const bt_summary* sum, const int32_t* sym_ids,
                        bt_param_agg* agg, bt_topk_rec* best);
int32_t bt_surface_merge(const bt_param_agg* in, int32_t world, int32_t P, bt_param_agg* out);
/* ---- walk-forward evaluation (k_walkfwd.hip, walkfwd.cpp; semantics: docs/walkforward_spec.md)
 * Every (symbol, param) lane of the resident dataset is walked once over its whole series and its
 * result is cut into K consecutive bar folds [bounds[k], bounds[k+1]) (absolute bar indices, clipped
 * to each row's bars, common to every row). A step j = max(train, 1) .. K-1 chooses, per row, the
 * parameter with the largest Sharpe over the training folds [j - train, j) ([0, j) when train == 0;
 * ties to the lowest param) and reports that lane's record of fold j, which the choice never saw.
 *   folds  [S][P][K] every lane's fold records (row-major), or NULL;
 *   steps  [S][K - max(train, 1)] one bt_wf_step per row and step, or NULL;
 *   total  [S] per row, the out-of-sample folds of its steps with param >= 0 as one record, or NULL.
 * Synchronous like bt_replay: waits for the engine's streams, runs on the engine stream, copies
 * back; bt_run need not have been called and nothing another entry point reads changes. Device
 * staging is bounded by a fixed 256 MB budget: the rows are processed in chunks, never S*P*K.
 * Added within ABI 3 (additive). Returns 0, or -1 with bt_last_error naming the offending value
 * (the engine stays usable): a null engine, no dataset, K < 1, bounds not strictly increasing or
 * bounds[0] < 0, train outside [0, K-1], steps or total with K < 2, all three outputs NULL, folds
 * with S*P*K > 2^22, one row's P*K records larger than the staging budget. */
typedef struct bt_fold {              /* 80 bytes */
    int32_t first_bar, n_bars, n_trades, status;
    int64_t pnl, mdd, exposure;       /* ticks, ticks, bars held */
    double  sharpe;
    uint64_t s1_lo; int64_t s1_hi; uint64_t s2_lo; int64_t s2_hi;  /* as bt_sums, of the fold */
} bt_fold;
typedef struct bt_wf_step {           /* 16 + 8 + 80 bytes */
    int32_t sym, fold, param, pad;    /* global id, the out-of-sample fold j, chosen param or -1 */
    double  train_sharpe;
    bt_fold oos;
} bt_wf_step;
int32_t bt_walk_forward(bt_engine* e, int32_t K, const int32_t* bounds /* K + 1 */, int32_t train,
                        bt_fold* folds, bt_wf_step* steps, bt_fold* total);
/* Device staging budget of bt_walk_forward in bytes: 0 = the default (256 MB). Results are
 * identical whatever the budget (tests force several chunks with a small one). */
int32_t bt_set_walkfwd_budget(bt_engine* e, int64_t bytes);
/* Host, no GPU needed: the steps and totals from fold records [S][P][K] (the scalar restatement of
 * the device selection). annualization is bt_config.annualization. steps and/or total (not both
 * NULL); K >= 2. */
int32_t bt_walk_forward_host(int32_t S, int32_t P, int32_t K, int32_t train, const bt_fold* folds,
                             const int32_t* sym_ids, int64_t annualization, bt_wf_step* steps,
                             bt_fold* total);
/* ---- portfolio of chosen lanes (k_portfolio.hip, portfolio.cpp; semantics: docs/portfolio_spec.md)
 * What the book does when n chosen lanes are traded together. Entry i is lane (sym, param) of the
 * resident dataset, walked once over its whole series, and counts on the bars [from_bar,
 * min(to_bar, its bars, T)); repeated entries count repeatedly, an empty window contributes nothing.
 *   pnl[t]      sum over the entries in window of E_t - E_(t-1) (E of spec §4, E_(-1) = 0), ticks;
 *   equity[t]   pnl[0] + .. + pnl[t];
 *   n_long[t], n_short[t]   entries in window with pos_t = +1 / -1;
 *   summary     one bt_pf_summary of the T bars.
 * Any output may be NULL, not all. Every figure is an integer sum or extremum: the bits do not
 * depend on the order of the entries, on the replica count or on how the entries are split over
 * shards (bt_portfolio_merge adds the parts). Synchronous like bt_replay: waits for the engine's
 * streams, runs on the engine stream, copies back; bt_run need not have been called and nothing
 * another entry point reads changes. Device staging is O(replicas * T + n), never n * T. Added
 * within ABI 3 (additive). Returns 0, or -1 with bt_last_error naming the offending index and value
 * (the engine stays usable): a null engine, no dataset, n < 0 or n > BT_PORTFOLIO_MAX, NULL lanes
 * with n > 0, T < 1 or T > 2^22, all outputs NULL, an unknown symbol id, param outside [0, P),
 * from_bar < 0, to_bar < from_bar, more than 2^30 window bars in all. n == 0 is legal: zero rows
 * and the zero summary. */
typedef struct bt_pf_lane {
    int32_t sym;                      /* global symbol id (bt_topk_rec.sym, bt_wf_step.sym) */
    int32_t param;
    int32_t from_bar, to_bar;         /* the entry counts on bars [from_bar, to_bar) */
} bt_pf_lane;
typedef struct bt_pf_summary {        /* 80 bytes */
    int32_t n_lanes;                  /* entries with a non-empty window */
    int32_t first_bar, n_bars;        /* lo and hi - lo: the bars some window covers (0, 0 without one) */
    int32_t max_gross;                /* max over t of n_long + n_short */
    int64_t pnl;                      /* equity[T - 1] */
    int64_t mdd;                      /* max over t of peak_t - equity[t], peak_t = max(0, equity[0..t]) */
    int64_t exposure;                 /* sum over t of n_long + n_short */
    double  sharpe;                   /* of the tick increments pnl[t] over [lo, hi) */
    uint64_t s1_lo; int64_t s1_hi; uint64_t s2_lo; int64_t s2_hi;  /* sum pnl[t], sum pnl[t]^2 */
} bt_pf_summary;
#define BT_PORTFOLIO_MAX (1 << 20)    /* entries per call */
int32_t bt_portfolio(bt_engine* e, int32_t n, const bt_pf_lane* lanes, int32_t T,
                     int64_t* pnl,      /* [T] or NULL */
                     int64_t* equity,   /* [T] or NULL */
                     int32_t* n_long,   /* [T] or NULL */
                     int32_t* n_short,  /* [T] or NULL */
                     bt_pf_summary* summary);
/* Replicas of the per-bar accumulators the walk adds into: 0 = the planner's choice, r = r (at
 * most 64, and as many as fit the accumulator budget). Results are identical either way. */
int32_t bt_set_portfolio_replicas(bt_engine* e, int32_t r);
/* Host, no GPU needed: the scalar restatement from per-entry curves as bt_replay returns them
 * (equity and pos rows of `stride` values, n_bars[i] bars each); lanes[i] gives entry i's window
 * (sym and param are not read). annualization is bt_config.annualization. */
int32_t bt_portfolio_host(int32_t n, const int64_t* equity, const int8_t* pos, const int32_t* n_bars,
                          int64_t stride, const bt_pf_lane* lanes, int32_t T, int64_t annualization,
                          int64_t* out_pnl, int64_t* out_equity, int32_t* out_long, int32_t* out_short,
                          bt_pf_summary* summary);
/* Host: `world` portfolios of disjoint entry sets over the same T bars as one. pnl, n_long and
 * n_short are [world][T] rows, summaries [world]; the rows add, first_bar / n_bars / n_lanes merge
 * by min / max / sum, and equity and the rest of the summary are recomputed from the merged rows
 * by the code bt_portfolio_host finishes with. Any output may be NULL, not all. */
int32_t bt_portfolio_merge(int32_t world, int32_t T, const int64_t* pnl, const int32_t* n_long,
                           const int32_t* n_short, const bt_pf_summary* summaries, int64_t annualization,
                           int64_t* out_pnl, int64_t* out_equity, int32_t* out_long, int32_t* out_short,
                           bt_pf_summary* summary);
/* ---- covariance of chosen lanes (k_gram.hip, covariance.cpp; semantics: docs/covariance_spec.md)
 * How n chosen lanes move together over one common window [from_bar, to_bar). With B_max the bars
 * of the longest requested symbol, to' = min(to_bar, B_max) and T = max(0, to' - from_bar), lane
 * i, walked once over its whole series, gives the increments d_t = E_t - E_(t-1) (E of spec §4,
 * E_(-1) = 0) on the window's bars below its own bar count and 0 on the others.
 *   gram[i*n + j]  sum over the window of d^i_t * d^j_t: an exact int128 (bt_wide, lo/hi words
 *                  like bt_sums), symmetric, |gram| < 2^84;
 *   sums[i]        sum over the window of d^i_t, int64 (below 2^53);
 *   T_out          T.
 * Every figure is an exact integer sum: the bits do not depend on the bar chunks the device cuts the
 * window into, and the grams of disjoint windows add to the gram of their union. The sum of all
 * gram entries is the s2 of the bt_portfolio of the same lanes over the same window, the sum of
 * sums its s1. Any output may be NULL, not all; with n == 0 or T == 0 every output is zero.
 * Synchronous like bt_replay: waits for the engine's streams, runs on the engine stream, copies
 * back; bt_run need not have been called and nothing another entry point reads changes. Added
 * within ABI 3 (additive). Returns 0, or -1 with bt_last_error naming the offending index and value
 * (the engine stays usable): a null engine, no dataset, n < 0 or n > BT_COV_MAX, NULL lanes with
 * n > 0, an unknown symbol id, param outside [0, P), from_bar < 0, to_bar < from_bar, T > 2^22, all
 * outputs NULL, a device staging need above 256 MB (n rows of T increments, the chunk partials and
 * the n x n result; the bytes are named). */
typedef struct bt_wide {              /* an int128: value = hi * 2^64 + lo */
    uint64_t lo;
    int64_t hi;
} bt_wide;
#define BT_COV_MAX 2048               /* lanes per call */
int32_t bt_covariance(bt_engine* e, int32_t n, const bt_lane* lanes, int32_t from_bar, int32_t to_bar,
                      bt_wide* gram,      /* [n * n] or NULL */
                      int64_t* sums,      /* [n] or NULL */
                      int32_t* T_out);    /* or NULL */
/* The same Gram kernels on a caller's increments d[n][T] (row-major int32, |d| < 2^31: INT32_MIN
 * is refused, with its index named): the way to the extremes of the exactness argument, which a
 * real series cannot reach. Works on any engine (also one without a dataset). n in [0, BT_COV_MAX],
 * T in [0, 2^22]; gram and/or sums (not both NULL). */
int32_t bt_gram_of(bt_engine* e, int32_t n, int32_t T, const int32_t* d, bt_wide* gram, int64_t* sums);
/* Bar chunks the Gram product is cut into (split-K): 0 = the planner's choice, k = k (at most one
 * per 64 bars). Results are identical either way. */
int32_t bt_set_gram_split(bt_engine* e, int32_t k);
/* Host, no GPU needed: the scalar restatement from replayed curves (equity rows of `stride` values,
 * n_bars[i] bars each, as bt_replay returns them). B_max is the largest n_bars[i]. */
int32_t bt_covariance_host(int32_t n, const int64_t* equity, const int32_t* n_bars, int64_t stride,
                           int32_t from_bar, int32_t to_bar, bt_wide* gram, int64_t* sums, int32_t* T_out);
/* ---- per-lane trade statistics and drawdown timing (k_tstats.hip, tstats.cpp; semantics:
 * docs/tradestats_spec.md). One bt_tstats per (symbol, param) lane, walked once over its whole
 * series: the counts, sums and extremes of its closed trades (pnl_i = side_i (exit_px_i -
 * entry_px_i), hold_i = exit_bar_i - entry_bar_i; a win has pnl_i > 0, a loss pnl_i < 0), the
 * longest runs of wins and of losses, and where the largest drawdown of the equity curve E_t of
 * spec §4 began and bottomed and how long the curve stayed below its running peak. Every figure is
 * an integer count, sum or extremum: exact, and independent of every order.
 *   list mode (lanes != NULL): the n lanes in request order, repeats allowed; bt_lane.sym is the
 *     global symbol id as in bt_replay. out[n] is required, agg must be NULL; n == 0 returns 0.
 *   all-lanes mode (lanes == NULL, n == 0): every lane of the resident dataset. out is [S * P]
 *     row-major or NULL, agg is [P] (one bt_tstats_agg per parameter over every dataset row) or
 *     NULL, not both NULL. With out == NULL nothing of size S x P leaves the device.
 * Synchronous like bt_replay: waits for the engine's streams, runs on the engine stream, copies
 * back; bt_run need not have been called and nothing another entry point reads changes. Device
 * staging is bounded by a 256 MB budget: rows (all-lanes mode) or lanes (list mode) go through in
 * chunks. Added within ABI 3 (additive). Returns 0, or -1 with bt_last_error naming the offending
 * value (the engine stays usable): a null engine, no dataset, n < 0 or n > BT_TSTATS_MAX, n != 0
 * with lanes == NULL, agg given in list mode, out missing in list mode, both outputs NULL, an
 * unknown symbol id, param outside [0, P), a budget smaller than one row's P records. */
typedef struct bt_tstats {            /* 128 bytes */
    int32_t n_trades, n_win, n_loss, status;        /* flat trades: n_trades - n_win - n_loss; status 0 */
    int32_t n_long, n_long_win;                     /* trades with side > 0, and the wins among them */
    int32_t max_win_streak, max_loss_streak;        /* longest runs in closing order; a flat trade ends both */
    int32_t hold_sum, hold_win, hold_max, n_bars;   /* sum of hold_i, over wins only, the largest; B */
    int64_t gross_win, gross_loss;                  /* sum of pnl_i over wins; of -pnl_i over losses (>= 0) */
    int64_t max_win, max_loss;                      /* largest pnl_i; largest -pnl_i over losses; 0 without one */
    uint64_t sq_lo; int64_t sq_hi;                  /* sum of pnl_i^2, an int128 as in bt_sums */
    int64_t mdd;                                    /* max over t of peak_t - E_t, peak_t = max(0, E_0..E_t) */
    int32_t mdd_bar, peak_bar;                      /* first bar at mdd; first bar at that bar's peak; -1, -1 when mdd == 0 */
    int32_t underwater_bars, max_underwater;        /* bars with E_t < peak_t; the longest run of them */
    uint64_t hash;                                  /* the trade hash of spec §4 */
} bt_tstats;
typedef struct bt_tstats_agg {        /* 136 bytes: one parameter over every dataset row */
    int32_t n_sym, n_traded;                        /* rows counted; rows with n_trades > 0 */
    int32_t max_win_streak, max_loss_streak, hold_max, max_underwater;   /* maxima over rows */
    int64_t n_trades, n_win, n_loss, n_long, n_long_win, hold_sum, hold_win, gross_win, gross_loss;  /* sums */
    int64_t max_win, max_loss, mdd_max;             /* maxima over rows */
    uint64_t sq_lo; int64_t sq_hi;                  /* int128 sum */
} bt_tstats_agg;
#define BT_TSTATS_MAX (1 << 20)       /* lanes per call in list mode */
int32_t bt_trade_stats(bt_engine* e, int32_t n, const bt_lane* lanes, bt_tstats* out, bt_tstats_agg* agg);
/* Device staging budget of bt_trade_stats in bytes: 0 = the default (256 MB). Results are
 * identical whatever the budget. */
int32_t bt_set_tstats_budget(bt_engine* e, int64_t bytes);
/* Host, no GPU needed: the scalar restatements. One lane's record from its complete trade list in
 * closing order and its equity curve (n_bars values, as bt_replay returns them); the reduction of
 * an S x P record matrix (row-major) to agg[P]; and the merge of `world` aggregates of P records
 * (in[w * P + p], disjoint row sets; world >= 1) into out[P]. */
int32_t bt_trade_stats_host(int32_t n_trades, const bt_trade* trades, int32_t n_bars,
                            const int64_t* equity, bt_tstats* out);
int32_t bt_tstats_agg_host(int32_t S, int32_t P, const bt_tstats* recs, bt_tstats_agg* agg);
int32_t bt_tstats_merge(const bt_tstats_agg* in, int32_t world, int32_t P, bt_tstats_agg* out);
/* ---- net of costs: every lane under a ladder of fee levels (k_costs.hip, costs.cpp; semantics:
 * docs/costs_spec.md). A call takes C in [1, BT_COST_LEVELS_MAX] levels, levels[2 j] = fixed_j in
 * [0, BT_COST_FIXED_MAX] ticks per fill and levels[2 j + 1] = bps_j in [0, BT_COST_BPS_MAX]; a fill
 * at price px pays fee_j(px) = fixed_j + floor(px * bps_j / 10000). Every trade of spec §4 has two
 * fills, its entry at entry_bar at entry_px and its exit at exit_bar at exit_px (a flip puts both on
 * one bar, a stop or target exit pays on the level price, the forced exit at B - 1 is a fill). With
 * f_t the fees of bar t's fills the net curve is N_t = E_t - sum of f_u over u <= t, and a trade's
 * net result is side (exit_px - entry_px) - fee_j(entry_px) - fee_j(exit_px). One bt_cost_rec per
 * (lane, level), levels innermost; every figure is an exact integer and level j's record depends on
 * level j alone.
 *   list mode (lanes != NULL): the n lanes in request order, repeats allowed. out[n * C] is
 *     required, agg must be NULL; n == 0 returns 0.
 *   all-lanes mode (lanes == NULL, n == 0): out is [S * P * C] or NULL, agg is [P * C] (one
 *     bt_cost_agg per (parameter, level) over every dataset row) or NULL, not both NULL. With out ==
 *     NULL nothing of size S x P leaves the device.
 * Synchronous like bt_trade_stats, and staged in chunks under a 256 MB budget in the same way.
 * Added within ABI 3 (additive). Returns 0, or -1 with bt_last_error naming the offending value
 * (the engine stays usable), checked in this order: a null engine, no dataset, C outside its range,
 * levels == NULL, a level outside its ranges (the level is named), n < 0 or n > BT_COSTS_MAX, n != 0
 * with lanes == NULL, agg given in list mode, out missing in list mode, both outputs NULL, an
 * unknown symbol id, param outside [0, P), a budget smaller than one row's P * C records. */
typedef struct bt_cost_rec {          /* 88 bytes */
    int32_t n_trades, n_win, n_loss, n_bars;        /* trades; those with net > 0; with net < 0; B */
    int32_t mdd_bar, underwater_bars;               /* first bar at the net mdd (-1 when it is 0); bars with N_t < peak_t */
    int64_t pnl, fees, turnover;                    /* N_(B-1); sum of f_t; sum of the fill prices */
    int64_t mdd;                                    /* max over t of peak_t - N_t, peak_t = max(0, N_0..N_t) */
    int64_t win_sum, loss_sum;                      /* sum of net_i over wins; of -net_i over losses */
    uint64_t s2_lo; int64_t s2_hi;                  /* sum over t of (N_t - N_(t-1))^2, an int128 as in bt_sums */
} bt_cost_rec;
typedef struct bt_cost_agg {          /* 48 bytes: one (parameter, level) over every dataset row */
    int32_t n_sym, n_traded, n_profit, pad;         /* rows; rows with n_trades > 0; rows with pnl > 0; 0 */
    int64_t trades, pnl, fees, mdd_max;             /* sums over the rows; the largest mdd */
} bt_cost_agg;
#define BT_COSTS_MAX (1 << 20)        /* lanes per call in list mode */
#define BT_COST_LEVELS_MAX 16
#define BT_COST_FIXED_MAX (1 << 20)
#define BT_COST_BPS_MAX 1000
int32_t bt_costs(bt_engine* e, int32_t C, const int32_t* levels, int32_t n, const bt_lane* lanes,
                 bt_cost_rec* out, bt_cost_agg* agg);
/* Device staging budget of bt_costs in bytes: 0 = the default (256 MB). Results are identical
 * whatever the budget. */
int32_t bt_set_costs_budget(bt_engine* e, int64_t bytes);
/* Host, no GPU needed: the scalar restatements. One lane's C records from its complete trade list
 * and its gross equity curve (n_bars values, as bt_replay returns them); the reduction of an
 * S x P x C record array (row-major) to agg[P * C]; and the merge of `world` aggregates of PC
 * records each (in[w * PC + q], disjoint row sets; world >= 1) into out[PC]. */
int32_t bt_costs_host(int32_t n_trades, const bt_trade* trades, int32_t n_bars, const int64_t* equity,
                      int32_t C, const int32_t* levels, bt_cost_rec* out);
int32_t bt_costs_agg_host(int32_t S, int32_t P, int32_t C, const bt_cost_rec* recs, bt_cost_agg* agg);
int32_t bt_costs_merge(const bt_cost_agg* in, int32_t world, int32_t PC, bt_cost_agg* out);
/* ---- tail risk: the shape of a lane's per-bar pnl (k_tail.hip, tail.cpp; semantics:
 * docs/tail_spec.md). Every lane is walked once over its whole series; its increments are d_t = E_t -
 * E_(t-1) with E_(-1) = 0, |d_t| < 2^31. The window is [from_bar, to_bar), from_bar = to_bar = 0
 * meaning the whole row; lane i contributes the n_window bars from_bar <= t < min(to_bar, B_i) (there
 * may be none). mode BT_TAIL_ALL counts every bar of the window, BT_TAIL_HELD only the bars a
 * position was held into (t >= 1 and pos_(t-1) != 0; on the other bars d_t is 0). Over the n counted
 * bars one bt_tail_rec per lane holds the counts, the extremes with the first bar that reaches each,
 * and the exact power sums up to the fourth; per (lane, level), levels innermost, one bt_tail_q
 * holds the lower-tail order statistics at alpha_ppm[j] in [1, 10^6] parts per million: with
 * k = ceil(n * alpha_ppm / 10^6), var is the k-th smallest counted d, es_sum the sum of the k
 * smallest and n_lt the number of counted d below var, so that es_sum = (sum of the d < var) +
 * (k - n_lt) * var. Q in [1, BT_TAIL_LEVELS_MAX] levels, in any order, repeats allowed; a level's
 * result depends on that level alone. With n = 0 both records are all zeros but min_bar = max_bar =
 * -1. Every figure is an exact integer, whatever the chunking, the budget or the home of the row.
 *   list mode (lanes != NULL): n in [1, BT_TAIL_MAX] lanes in request order, repeats allowed;
 *     recs_out[n], q_out[n * Q].
 *   all-lanes mode (lanes == NULL, n == 0): recs_out[S * P], q_out[S * P * Q].
 * Either output may be NULL, not both. Synchronous; bt_run need not have been called. Added within
 * ABI 3 (additive). Returns 0, or -1 with bt_last_error naming the offending value (the engine stays
 * usable), checked in this order: a null engine, no dataset, n, Q, alpha_ppm == NULL, a level outside
 * its range (the level is named), mode, the window, both outputs NULL, a dataset row longer than
 * BT_TAIL_BARS_MAX, an unknown symbol id, param outside [0, P), a row that does not fit LDS under
 * bt_set_tail_row(e, 1), a staging need above the budget (the bytes are named). */
typedef struct bt_tail_rec {          /* 128 bytes */
    int32_t n, n_window, n_pos, n_neg;              /* counted bars; bars of the window; counted d > 0; d < 0 */
    int32_t min_bar, max_bar;                       /* the smallest t that reaches min_d / max_d (-1 when n = 0) */
    int64_t min_d, max_d, s1, s1_neg;               /* extremes; sum of d; sum of min(d, 0) */
    bt_wide s2, s2_neg, s3;                         /* sum of d^2; of min(d, 0)^2; of d^3 (signed) */
    uint64_t s4[3];                                 /* sum of d^4, 192 bits, least significant word first */
} bt_tail_rec;
typedef struct bt_tail_q {            /* 24 bytes */
    int64_t var, es_sum;                            /* the k-th smallest counted d; the sum of the k smallest */
    int32_t k, n_lt;                                /* ceil(n alpha / 10^6); counted d < var */
} bt_tail_q;
enum bt_tail_mode { BT_TAIL_ALL = 0, BT_TAIL_HELD = 1 };
#define BT_TAIL_MAX (1 << 20)         /* lanes per call in list mode, rows of bt_tail_of */
#define BT_TAIL_LEVELS_MAX 8
#define BT_TAIL_PPM_MAX 1000000
#define BT_TAIL_BARS_MAX (1 << 22)    /* bars of a row */
int32_t bt_tail(bt_engine* e, int32_t n, const bt_lane* lanes, int32_t from_bar, int32_t to_bar, int32_t mode,
                int32_t Q, const int32_t* alpha_ppm, bt_tail_rec* recs_out, bt_tail_q* q_out);
/* The same kernels on a caller's increments d[n][T] (row-major int32, |d| < 2^31: INT32_MIN is
 * refused with its index), n in [1, BT_TAIL_MAX], T in [1, BT_TAIL_BARS_MAX]. Every entry is counted
 * and min_bar / max_bar are indices into the row. Needs no dataset. */
int32_t bt_tail_of(bt_engine* e, int32_t n, int32_t T, const int32_t* d, int32_t Q, const int32_t* alpha_ppm,
                   bt_tail_rec* recs_out, bt_tail_q* q_out);
/* Where a lane's row of counted increments lives during the selection: 0 = the planner's choice, 1 =
 * LDS (a call whose longest row does not fit is refused), 2 = device memory. bt_set_tail_budget: the
 * device staging budget in bytes, 0 = the default (256 MB). Results are identical under every
 * setting. bt_last_tail_row: the home the last bt_tail / bt_tail_of of this engine used (1 or 2; 0
 * before the first). */
int32_t bt_set_tail_row(bt_engine* e, int32_t mode);
int32_t bt_set_tail_budget(bt_engine* e, int64_t bytes);
int32_t bt_last_tail_row(bt_engine* e);
/* Host, no GPU needed: the scalar restatement from replayed curves, n lanes with equity rows of
 * `stride` values, n_bars[i] of them meaningful, and the pos rows bt_replay returns (pos may be NULL
 * with mode BT_TAIL_ALL only). It sorts a copy of every row. */
int32_t bt_tail_host(int32_t n, const int64_t* equity, const int8_t* pos, const int32_t* n_bars, int64_t stride,
                     int32_t from_bar, int32_t to_bar, int32_t mode, int32_t Q, const int32_t* alpha_ppm,
                     bt_tail_rec* recs_out, bt_tail_q* q_out);
/* ---- bootstrap reality check (k_boot.hip, bootstrap.cpp; semantics: docs/bootstrap_spec.md).
 * Is the best lane of a group luck? n lanes in G groups (group g holds lanes goff[g] .. goff[g+1] - 1)
 * over one window [from_bar, to_bar) of T = to_bar - from_bar bars (to_bar is NOT clipped to a row's
 * bars, so that T and the resample plan do not depend on the rows a shard holds; from_bar = to_bar
 * = 0 means [0, B_max), B_max the bars of the longest requested row, in all-lanes mode of the
 * longest dataset row). Lane i, walked once over its whole series, gives d^i_k = E_(from+k) -
 * E_(from+k-1) on the window's bars below its bar count and 0 elsewhere. A circular block bootstrap
 * with blocks of L' = min(L, T) bars (K = ceil(T / L') blocks, the last one truncated so that every
 * resample draws T bars) resamples all lanes jointly B times: block j of resample b starts at draw
 * j (0-based) of the SplitMix64 generator of docs/oracle_spec.md §1 keyed by (seed, b), taken
 * modulo T as an unsigned 64-bit number. S*_(i,b) is lane i's resampled sum, S_i its plain sum.
 *   lanes_out[i]   bt_boot_lane: sum = S_i, n_nonpos = #{b : S* <= 0}, m1 = sum over b of S*,
 *                  m2 = sum over b of S*^2 (bt_wide: m1 can pass 2^63);
 *   groups_out[g]  bt_boot_group: best_sum = max S_i over the group, best_lane the lowest index
 *                  inside the group that reaches it, n_lanes, and n_ge = #{b : V*_(g,b) >= best_sum}
 *                  with V*_(g,b) = max over the group of S*_(i,b) - S_i: n_ge / B is White's p-value;
 *   vmax_out       [G * B] the V*;  boot_out  [n * B] the raw S* (list mode only).
 * Every figure is an exact integer (|S*| < 2^53); per-group results of shards concatenate.
 *   list mode (lanes != NULL): n in [1, BT_BOOT_MAX] lanes, repeats allowed; goff == NULL means
 *     one group (G is then 0 or 1).
 *   all-lanes mode (lanes == NULL, n == 0, goff == NULL, G == 0): every dataset row's P lanes are
 *     one group, in dataset order: groups_out[S], lanes_out[S * P], vmax_out[S * B]; boot_out must
 *     be NULL.
 * Any output may be NULL, not all. Synchronous like bt_replay; bt_run need not have been called and
 * nothing another entry point reads changes. Added within ABI 3 (additive). Returns 0, or -1 with
 * bt_last_error naming the offending value (the engine stays usable): a null engine, no dataset, n
 * outside its range, goff that does not start at 0, increase strictly or end at n, an unknown
 * symbol id, param outside [0, P), from_bar < 0, T < 1 or T > 2^22, B outside [1, 65536], L
 * outside [1, 2^22], all outputs NULL, boot_out in all-lanes mode, a device staging need above
 * the budget (the bytes are named: the start table K*B*4, vmax G*B*8, the per-lane records, a
 * requested boot and, when the prefix rows live in device memory, one row). */
typedef struct bt_boot_lane {         /* 48 bytes */
    int64_t sum;                                    /* S_i */
    int64_t n_nonpos;                               /* resamples with S* <= 0 */
    bt_wide m1, m2;                                 /* sum of S*, sum of S*^2 over the B resamples */
} bt_boot_lane;
typedef struct bt_boot_group {        /* 24 bytes */
    int64_t best_sum;
    int32_t best_lane, n_lanes;                     /* best_lane counts from the group's first lane */
    int64_t n_ge;
} bt_boot_group;
#define BT_BOOT_MAX (1 << 20)         /* lanes per call in list mode and of bt_bootstrap_of */
#define BT_BOOT_MAX_RESAMPLES 65536
int32_t bt_bootstrap(bt_engine* e, int32_t n, const bt_lane* lanes, int32_t G, const int32_t* goff,
                     int32_t from_bar, int32_t to_bar, int32_t B, int32_t L, uint64_t seed,
                     bt_boot_group* groups_out,   /* [G] or NULL */
                     bt_boot_lane* lanes_out,     /* [n] or NULL */
                     int64_t* vmax_out,           /* [G * B] or NULL */
                     int64_t* boot_out);          /* [n * B] or NULL */
/* The same resampling and finish on a caller's increments d[n][T] (row-major int32, |d| < 2^31:
 * INT32_MIN is refused, with its index named): the way to the ends of the range argument. Works on
 * any engine (also one without a dataset). n in [1, BT_BOOT_MAX], T in [1, 2^22]. */
int32_t bt_bootstrap_of(bt_engine* e, int32_t n, int32_t T, const int32_t* d, int32_t G, const int32_t* goff,
                        int32_t B, int32_t L, uint64_t seed, bt_boot_group* groups_out, bt_boot_lane* lanes_out,
                        int64_t* vmax_out, int64_t* boot_out);
/* Device staging budget of the two calls in bytes: 0 = the default (256 MB). Results are identical
 * whatever the budget. */
int32_t bt_set_boot_budget(bt_engine* e, int64_t bytes);
/* Where a lane's prefix row lives while it is resampled: 0 = the planner's choice, 1 = in LDS
 * (refused at call time when the row of T + 1 words does not fit), 2 = in device memory. Results
 * are identical either way. */
int32_t bt_set_boot_row(bt_engine* e, int32_t mode);
/* Host, no GPU needed: the scalar restatement from replayed curves (equity rows of `stride` values,
 * n_bars[i] bars each, as bt_replay returns them), which adds the drawn bars one by one. goff ==
 * NULL means one group; from_bar = to_bar = 0 means [0, max n_bars). */
int32_t bt_bootstrap_host(int32_t n, const int64_t* equity, const int32_t* n_bars, int64_t stride, int32_t G,
                          const int32_t* goff, int32_t from_bar, int32_t to_bar, int32_t B, int32_t L,
                          uint64_t seed, bt_boot_group* groups_out, bt_boot_lane* lanes_out, int64_t* vmax_out,
                          int64_t* boot_out);
/* ---- drawdown bootstrap (k_ddboot.hip, ddboot.cpp; semantics: docs/drawdown_spec.md).
 * How deep could each lane's drawdown be? The circular block bootstrap of bt_bootstrap (the same
 * window rule, T, L', K, truncated last block, draws and modulo: a call with the same window, B, L
 * and seed draws the same bars) applied to a path functional: MDD(x) = max over m of (peak_m - X_m),
 * X_m the sum of the first m values, peak_m = max(0, X_1 .. X_m). Per lane mdd = MDD of the
 * window's increments (with the default window the run's summary mdd), and MDD*_(i,b) = MDD of the
 * T bars resample b draws, 0 <= MDD* < 2^53.
 *   lanes_out[i]     bt_dd_lane: sum = S_i, mdd, n_ge = #{b : MDD* >= mdd}, min_star and max_star
 *                    over b, m1 = sum over b of MDD*, m2 = sum over b of MDD*^2;
 *   q_out[i*Q + j]   the k_j-th smallest MDD* of lane i, k_j = ceil(B * alpha_ppm[j] / 10^6);
 *   reach_out[i*R+r] #{b : MDD* >= limits[r]};
 *   raw_out[i*B + b] the raw MDD* (list mode and bt_drawdown_boot_of only).
 * Q in [0, BT_DD_LEVELS_MAX] levels in [1, 10^6] ppm, R in [0, BT_DD_LIMITS_MAX] limits >= 0 in
 * ticks, in any order, repeats allowed. There are no groups: every figure depends on its lane
 * alone, so shards called with one explicit window concatenate.
 *   list mode (lanes != NULL): n in [1, BT_BOOT_MAX] lanes in request order, repeats allowed;
 *   all-lanes mode (lanes == NULL, n == 0): every lane of the dataset, row-major [S][P]; raw_out
 *     must be NULL.
 * Any output may be NULL, not all (q_out counts with Q > 0, reach_out with R > 0). Synchronous like
 * bt_replay; nothing another entry point reads changes. Added within ABI 3 (additive). Returns 0, or
 * -1 with bt_last_error naming the offending value (the engine stays usable): bt_bootstrap's own
 * refusals of the engine, the dataset, n, the lanes, from_bar, T, B and L, Q or R outside [0, 8], a
 * level or a limit out of range (its index named), all outputs NULL, raw_out in all-lanes mode, a
 * staging need above the budget (the bytes named), a row that does not fit LDS under
 * bt_set_ddboot_row(e, 1). */
typedef struct bt_dd_lane {           /* 72 bytes */
    int64_t sum;                                    /* S_i */
    int64_t mdd;                                    /* the observed largest drawdown */
    int64_t n_ge;                                   /* resamples with MDD* >= mdd */
    int64_t min_star, max_star;                     /* smallest and largest MDD* */
    bt_wide m1, m2;                                 /* sum of MDD*, sum of MDD*^2 over the B resamples */
} bt_dd_lane;
#define BT_DD_LEVELS_MAX 8
#define BT_DD_LIMITS_MAX 8
int32_t bt_drawdown_boot(bt_engine* e, int32_t n, const bt_lane* lanes, int32_t from_bar, int32_t to_bar, int32_t B,
                         int32_t L, uint64_t seed, int32_t Q, const int32_t* alpha_ppm, int32_t R,
                         const int64_t* limits,
                         bt_dd_lane* lanes_out,       /* [n] or NULL */
                         int64_t* q_out,              /* [n * Q] or NULL */
                         int64_t* reach_out,          /* [n * R] or NULL */
                         int64_t* raw_out);           /* [n * B] or NULL */
/* The same on a caller's increments d[n][T] (row-major int32, INT32_MIN refused with its index),
 * on any engine (also one without a dataset). n in [1, BT_BOOT_MAX], T in [1, 2^22]. */
int32_t bt_drawdown_boot_of(bt_engine* e, int32_t n, int32_t T, const int32_t* d, int32_t B, int32_t L, uint64_t seed,
                            int32_t Q, const int32_t* alpha_ppm, int32_t R, const int64_t* limits,
                            bt_dd_lane* lanes_out, int64_t* q_out, int64_t* reach_out, int64_t* raw_out);
/* bt_set_ddboot_budget: the device staging budget in bytes, 0 = the default (256 MB).
 * bt_set_ddboot_row: where a lane's prefix row and block tables live: 0 = the planner's choice, 1 =
 * LDS (a call whose row does not fit is refused), 2 = device memory. Results are identical under
 * every setting. bt_last_ddboot_row: the home the last call of this engine used (1 or 2; 0 before
 * the first). */
int32_t bt_set_ddboot_budget(bt_engine* e, int64_t bytes);
int32_t bt_set_ddboot_row(bt_engine* e, int32_t mode);
int32_t bt_last_ddboot_row(bt_engine* e);
/* Host, no GPU needed: the scalar restatement from replayed curves (equity rows of `stride` values,
 * n_bars[i] bars each), which adds the drawn bars one by one and walks every resampled path: no
 * prefix row, no block table. from_bar = to_bar = 0 means [0, max n_bars). It sorts every lane's B
 * values. */
int32_t bt_drawdown_boot_host(int32_t n, const int64_t* equity, const int32_t* n_bars, int64_t stride, int32_t from_bar,
                              int32_t to_bar, int32_t B, int32_t L, uint64_t seed, int32_t Q, const int32_t* alpha_ppm,
                              int32_t R, const int64_t* limits, bt_dd_lane* lanes_out, int64_t* q_out,
                              int64_t* reach_out, int64_t* raw_out);
/* ---- probability of backtest overfitting (k_cscv.hip, cscv.cpp; semantics: docs/cscv_spec.md).
 * How often does "pick the best lane in-sample" choose a lane that is below the median out of
 * sample? Combinatorially symmetric cross-validation over the fold records of bt_walk_forward: the
 * series is cut into K folds (K even, 2 <= K <= BT_CSCV_MAX_FOLDS) by bounds[K + 1] as there, and
 * every one of the C = binom(K, K/2) ways of taking K/2 folds as the in-sample half is a
 * combination; combination c has the c-th K-bit mask with K/2 bits set in increasing numeric order
 * (bit k = fold k in-sample). A group is one dataset row's P lanes. Per group and combination the
 * lane p* with the largest in-sample Sharpe (exact int128 sums over the half's folds, ties to the
 * lowest p) is ranked among the group's lanes on the other half: r2 = 2 * #{below} + #{equal, not
 * p*} in [0, 2(P-1)]. The combination is overfit when r2 <= P - 1, a loss when p*'s out-of-sample
 * sum of returns is negative, tied when another lane shares p*'s in-sample Sharpe, and dead (no
 * pick, counted in n_dead only) when either half has no return bar.
 *   groups [G]          one bt_cscv_group per row (G = S), or NULL;
 *   hist   [G][2P - 1]  live combinations per r2, or NULL;
 *   picks  [G][C]       one bt_cscv_pick per combination (lane -1 when dead), or NULL; G*C <= 2^22.
 * Every figure is an integer or one Sharpe double: nothing depends on chunking or launch splitting.
 * Synchronous like bt_walk_forward, whose row chunks and staging budget (bt_set_walkfwd_budget) it
 * uses; bt_run need not have been called and nothing another entry point reads changes. Added
 * within ABI 3 (additive). Returns 0, or -1 with bt_last_error naming the offending value (the
 * engine stays usable): a null engine, no dataset, K odd or outside [2, 20], bounds as in
 * bt_walk_forward, all three outputs NULL, picks with G*C > 2^22, one row larger than the budget. */
#define BT_CSCV_MAX_FOLDS 20
typedef struct bt_cscv_group {        /* 32 bytes */
    int32_t sym, n_lanes;             /* the row's global id (staged: sym_ids[g], or g); P */
    int32_t n_live, n_dead;           /* combinations with a pick; without: n_live + n_dead = C */
    int32_t n_overfit, n_loss, n_tied;
    int32_t pad;
} bt_cscv_group;
typedef struct bt_cscv_pick {         /* 24 bytes */
    int32_t lane, r2;                 /* p* (-1: dead), its out-of-sample rank r2 */
    double  is_sharpe, oos_sharpe;    /* p*'s Sharpe on the in-sample and on the other half */
} bt_cscv_pick;
int32_t bt_cscv(bt_engine* e, int32_t K, const int32_t* bounds /* K + 1 */, bt_cscv_group* groups,
                uint32_t* hist, bt_cscv_pick* picks);
/* The same kernels on a caller's fold records folds[G][P][K] (for example the folds of
 * bt_walk_forward): G groups of P lanes. Only first_bar, n_bars and the s1/s2 words of a record
 * are read. sym_ids[G] or NULL (then group g reports sym = g). Works on any engine (also one
 * without a dataset). Also refused: P < 1, G < 0 (G == 0 writes nothing), NULL folds with G > 0, a
 * group whose lanes disagree in first_bar or n_bars of some fold (group, lane and fold are named),
 * first_bar or n_bars below 0 or a group of 2^31 - 1 return bars or more, and a record with s2 < 0,
 * s2 >= 2^120 or |s1| >= 2^120 (so that 20 of them stay inside an int128). */
int32_t bt_cscv_of(bt_engine* e, int32_t G, int32_t P, int32_t K, const bt_fold* folds,
                   const int32_t* sym_ids, bt_cscv_group* groups, uint32_t* hist, bt_cscv_pick* picks);
/* Host, no GPU needed: the scalar restatement. annualization is bt_config.annualization. */
int32_t bt_cscv_host(int32_t G, int32_t P, int32_t K, const bt_fold* folds, const int32_t* sym_ids,
                     int64_t annualization, bt_cscv_group* groups, uint32_t* hist, bt_cscv_pick* picks);
/* The most (row, combination pair, lane) cells one launch of the combination kernel covers: 0 =
 * the default. A chunk is cut into launches of whole rows or, where one row has more, of a row's
 * pairs. Results are identical whatever the value (tests force many launches with a small one). */
int32_t bt_set_cscv_work(bt_engine* e, int64_t cells);
/* Average device time of the dominant kernel (BT_FLAG_TIMING), and how many launches. */
int32_t bt_kernel_timing(bt_engine* e, double* total_ms, int64_t* launches, const char** name);
int32_t bt_reset_timing(bt_engine* e);
/* Profiling aid of the developer build libbt_prof.so only (`make PROFILING=1`, env BT_ABLATE=64):
 * per-phase s_memtime sums of the last run (n <= 32). The release libbt.so reads no environment
 * variable and always returns -1 ("no debug stamps") here. */
int32_t bt_read_debug(bt_engine* e, uint64_t* out, int32_t n);

/* ---- top-k merge (host): merge sorted record lists from several shards (RCCL gather). */
int32_t bt_merge_topk(const bt_topk_rec* in, size_t n, int32_t k, bt_topk_rec* out);

/* ---- multi-GPU exchange (comm.cpp): one process per GPU, each running its own
 * symbol shard; per run ONE RCCL all-gather over xGMI of every rank's top-k records and
 * counters, straight from the engine's device buffers. Replaces nothing in the reference, whose
 * only parallelism is job farming over gRPC (/root/reference/src/server/main.rs:131-143).
 *   rank 0: bt_comm_unique_id(id); the launcher broadcasts the 128 bytes; every rank:
 *   bt_comm_create(id, rank, world, device, k) — a collective call, all ranks together.
 * bt_exchange_async enqueues the exchange of the engine's last run (which needs topk >= k) into
 * pinned slot 0 .. BT_PIPE_SLOTS-1 behind the run's top-k chain, without a host wait;
 * bt_exchange_wait returns the merged global top-k (count) and counters[2] = {bar-evals, trades}
 * summed over ranks.
 * Every rank must issue the same sequence of exchanges.
 * RCCL is loaded at run time (dlopen of librccl.so.1 on the first bt_comm_unique_id /
 * bt_comm_create): libbt.so does not link it, so a single-GPU host loads the engine without RCCL,
 * and these two calls fail with "RCCL is not loadable" there. */
#define BT_COMM_ID_BYTES 128
typedef struct bt_comm bt_comm;
int32_t bt_comm_unique_id(uint8_t* out);
bt_comm* bt_comm_create(const uint8_t* id, int32_t rank, int32_t world, int32_t device, int32_t k,
                        char* err, size_t errlen);
void bt_comm_destroy(bt_comm* c);
int32_t bt_exchange_async(bt_comm* c, bt_engine* e, int32_t slot);
int32_t bt_exchange_wait(bt_comm* c, int32_t slot, bt_topk_rec* out, int32_t k,
                         int64_t* counters);
/* The host half of bt_exchange_wait, callable without a GPU: `block` (block_bytes long, which
 * must equal world * bt_exchange_message_bytes(k_msg), else -1) holds `world` messages in rank
 * order, each [header record whose first int32 is
 * the record count n (clipped to k_msg; < 0 is an error) | k_msg records, the first n sorted |
 * int64 bar-evals | int64 trades], as the all-gather delivers them. Writes the min(k, k_msg,
 * sum n) best records in engine order and counters[2] = the summed counters; returns the count. */
int64_t bt_exchange_message_bytes(int32_t k_msg);
int32_t bt_exchange_merge(const uint8_t* block, size_t block_bytes, int32_t world, int32_t k_msg,
                          bt_topk_rec* out, int32_t k, int64_t* counters);

/* ---- self-test hooks (host-side helpers the tests call without a GPU) */
/* The CompleteRequest.data text of P summaries (spec §6, one JSON line per param), as
 * bt_run_batch writes it; returns its length, or the capacity needed when out is NULL. */
int64_t bt_format_summaries(const bt_summary* r, int32_t P, char* out, size_t cap);
double bt_i128_to_double(uint64_t lo, int64_t hi);
int32_t bt_parse_csv(const uint8_t* buf, size_t len, int32_t cap, int32_t* h, int32_t* l,
                     int32_t* c, char* err, size_t errlen);   /* same as bt_parse_job */
/* Host ingest of one Job.File (CSV or binary columns) into h/l/c ticks;
 * returns the bar count, or -1 with the message in err. */
int32_t bt_parse_job(const uint8_t* buf, size_t len, int32_t cap, int32_t* h, int32_t* l,
                     int32_t* c, char* err, size_t errlen);

/* ---- binary columnar Job.File payload (payload.cpp): "DBXCOL1\n", u32 n_bars, u32 flags
 * (bit 0: int64 volume follows), then int32 open/high/low/close columns. Both return the byte
 * size (the required size when out is NULL) or -1. */
int64_t bt_encode_columns(const int32_t* o, const int32_t* h, const int32_t* l, const int32_t* c,
                          const int64_t* v, int32_t n, uint8_t* out, size_t cap);
/* Spec §1 synthetic OHLCV of one symbol generated on the host as a binary payload (the
 * dispatcher-side producer for gRPC-fed runs; bit-identical to bt_load_synthetic). */
int64_t bt_gen_payload(uint64_t seed, int64_t sym, int32_t bars, int32_t freq, uint8_t* out,
                       size_t cap);

#ifdef __cplusplus
}
#endif
#endif
