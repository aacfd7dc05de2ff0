// engine.cpp — the C ABI of include/bt.h but its analysis calls (analysis.cpp): engine lifecycle
// (the engine itself is engine_state.h), HBM-resident datasets, runs and read-backs, the
// JobsReply batch entry point (drop-in for process_incoming_job,
// /root/reference/src/worker/process.rs:13-29); its host half, ingest and result strings, is batch.cpp.
//
// Nothing here computes a backtest on the CPU: every result comes from the HIP kernels in
// k_*.hip. The host moves bars to HBM, launches and reads back; the HIP objects it holds are the
// self-freeing types of hip_owned.h.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "batch.h"
#include "csv.h"
#include "engine_state.h"
#include "topk_rules.h"

using namespace bt;

static thread_local std::string g_err;

void bt::set_last_error(const std::string& s) { g_err = s; }

namespace {

const char* kernel_name(int32_t strategy) {
    switch (strategy) {
        case BT_SMA_CROSS: return "bt::sma_kernel";
        case BT_EMA_OLS: return "bt::ema_tile_kernel";
        default: return "bt::boll_tile_kernel";
    }
}

std::string validate_and_copy(bt_engine* e, const bt_config& c) {
    const std::string err = plan_grid(c, e->grid);
    if (!err.empty()) return err;
    AxisSpec ax[4];
    const int nax = config_axes(c, ax);
    for (int i = 0; i < nax; ++i) e->ax[i].assign(ax[i].v, ax[i].v + ax[i].n);
    e->P = e->grid.n_params;
    if (c.annualization <= 0) return "annualization must be positive";
    e->grid.sqrt_ann = std::sqrt((double)c.annualization);
    if (c.topk < 0 || c.topk > kTopkMax) return "topk must be in [0, 1024]";
    if ((c.flags & BT_FLAG_PARITY) && c.trade_cap <= 0) return "parity mode needs trade_cap > 0";
    return "";
}

void upload_grid(bt_engine* e) {
    const int32_t** dst[4] = {&e->grid.a, &e->grid.b, &e->grid.c, &e->grid.d};
    for (int i = 0; i < 4; ++i) {
        *dst[i] = nullptr;
        if (e->ax[i].empty()) continue;
        e->d_axes[i].ensure(e->ax[i].size());
        HIPCHK(hipMemcpy(e->d_axes[i].p, e->ax[i].data(), e->ax[i].size() * 4, hipMemcpyHostToDevice));
        *dst[i] = e->d_axes[i].p;
    }
    e->grid.kwin = nullptr;
    e->grid.krecip = nullptr;
    if (e->cfg.strategy == BT_SMA_CROSS) {  // the key tasks' window table (internal.h Grid::kwin)
        std::vector<int32_t> win(e->ax[0]);
        win.insert(win.end(), e->ax[1].begin(), e->ax[1].end());
        win.resize((win.size() + kKeyGrab - 1) / kKeyGrab * kKeyGrab, 1);
        std::vector<double> recip(win.size());
        for (size_t i = 0; i < win.size(); ++i) recip[i] = key_recip(win[i]);
        e->d_kwin.ensure(win.size());
        e->d_krecip.ensure(win.size());
        HIPCHK(hipMemcpy(e->d_kwin.p, win.data(), win.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(e->d_krecip.p, recip.data(), recip.size() * sizeof(double), hipMemcpyHostToDevice));
        e->grid.kwin = e->d_kwin.p;
        e->grid.krecip = e->d_krecip.p;
    }
}

static_assert(kStageAlign == kRowAlign, "batch.h lays staging rows out as the device columns");

// Install a dataset: symbol descriptors (row offsets into the columns) and `rows` rows per
// column; allocates the columns the strategy needs.
void set_dataset(bt_engine* e, std::vector<SymDesc>&& syms, int64_t rows) {
    // the previous run's top-k chain (second stream) reads the symbol descriptors (ids of its
    // records), and a column may be reallocated below: every stream drains first (the upload on
    // the engine stream alone would be ordered after the kernel but not after that chain)
    sync_all(e);
    e->syms = std::move(syms);
    e->rows = rows;
    e->max_bars = 0;
    for (const SymDesc& sd : e->syms) e->max_bars = std::max(e->max_bars, sd.bars);
    const size_t n_sym = e->syms.size();
    e->d_syms.ensure(std::max<size_t>(1, n_sym));
    if (n_sym)
        HIPCHK(hipMemcpyAsync(e->d_syms.p, e->syms.data(), n_sym * sizeof(SymDesc),
                              hipMemcpyHostToDevice, main_stream(e)));
    const size_t r = std::max<int64_t>(1, rows);
    e->d_c.ensure(r);
    if (has_hl(e)) {
        e->d_h.ensure(r);
        e->d_l.ensure(r);
    }
    e->ran = false;
}

// Lay out rows (64-element aligned) and allocate the columns the strategy needs.
void layout(bt_engine* e, int32_t n_sym, const int32_t* bars, const int64_t* ids) {
    std::vector<SymDesc> syms((size_t)n_sym);
    int64_t off = 0;
    for (int32_t s = 0; s < n_sym; ++s) {
        syms[s].off = off;
        syms[s].bars = bars[s];
        syms[s].id = (int32_t)ids[s];
        off += align_rows(bars[s]);
    }
    set_dataset(e, std::move(syms), off);
}

TopkWork topk_work(bt_engine* e) {
    return TopkWork{e->d_hist.p, e->d_state.p, e->d_counts.p, e->d_above.p, e->d_cand.p,
                    kTopkCap, e->d_top.p + 1, reinterpret_cast<int32_t*>(e->d_top.p)};
}

void ensure_outputs(bt_engine* e) {
    const size_t n = (size_t)e->syms.size() * e->P;
    for (int b = 0; b < 2; ++b) {
        e->d_sum[b].ensure(std::max<size_t>(1, n));
        e->d_key[b].ensure(std::max<size_t>(1, n));
    }
    e->d_ntr_ring.ensure(kNtrRing);
    if (e->cfg.flags & BT_FLAG_PARITY) {
        e->d_sums.ensure(std::max<size_t>(1, n));
        e->d_trades.ensure(std::max<size_t>(1, n * (size_t)e->cfg.trade_cap));
    }
    if (e->cfg.topk > 0 && !e->topk_ready) {
        e->d_hist.ensure(4096);
        e->d_counts.ensure(2);
        e->d_state.ensure(4);
        e->d_above.ensure(kTopkCap);
        e->d_cand.ensure(kTopkCap);
        e->d_top.ensure(kTopkMax + 1);  // [0] = header (record count), then the records
        e->h_top.ensure(kTopkMax + 1);
        HIPCHK(launch_topk_init(topk_work(e), main_stream(e)));
        e->topk_ready = true;
    }
}

// Orders the run stream behind what the engine stream holds now, if main_stream() handed it out
// since the last time.
void run_stream_follows_main(bt_engine* e) {
    if (!e->main_dirty || !e->rstream) return;
    HIPCHK(hipEventRecord(e->ev_main, e->stream));
    HIPCHK(hipStreamWaitEvent(e->rstream, e->ev_main, 0));
    e->main_dirty = false;
}

void run_impl(bt_engine* e) {
    activate(e);
    ensure_outputs(e);
    const int32_t S = (int32_t)e->syms.size();
    const bool parity = (e->cfg.flags & BT_FLAG_PARITY) != 0;
    const LaunchPlan pl = plan_launch(e->grid, e->ax[0].data(),
                                      RunShape{S, e->max_bars, parity, e->seg_req, e->burn_req, e->cus,
                                               e->stream.owned, e->overlap_on});
    const int64_t run = e->nrun++;
    const int b = (int)(run & 1);
    e->cur = b;
    const int slot = (int)(run % kNtrRing);
    if (slot % (kNtrRing / 2) == 0) {
        // the half ring's last writers ran on either stream and the runs that add into it next
        // will too: zeroed on the engine stream behind the run stream's last kernel, and the run
        // stream ordered behind the zeroing at once, not behind this run's kernel. Its last
        // readers (tstream, 33 or more runs back) ended before the ev_tdone a later run waited for
        HIPCHK(hipMemsetAsync(e->d_ntr_ring.p + slot, 0, (kNtrRing / 2) * sizeof(unsigned long long),
                              main_stream(e)));
        run_stream_follows_main(e);
    }
    // A run that may overlap its neighbours (plan.h) goes to the stream of its output buffer: even
    // runs to the engine stream, odd ones to the run stream, so run i+1's blocks take the slots run
    // i's last blocks free. Any other run goes to the engine stream behind both streams' kernels,
    // and the run after it behind it
    const bool on_run = pl.overlap && b == 1;
    if (on_run) run_stream_follows_main(e);
    const hipStream_t st = on_run ? (hipStream_t)e->rstream : pl.overlap ? (hipStream_t)e->stream : main_stream(e);
    // buffer b was last read by the top-k chain / read-back of run i-2: wait for them (no wait
    // packet when they have already finished, the steady state of a pipelined sweep)
    if (e->tdone_armed[b] && hipEventQuery(e->ev_tdone[b]) != hipSuccess)
        HIPCHK(hipStreamWaitEvent(st, e->ev_tdone[b], 0));
    Out out{};
    out.sum = e->d_sum[b].p;
    out.key = e->d_key[b].p;
    out.sums = parity ? e->d_sums.p : nullptr;
    out.trades = parity ? e->d_trades.p : nullptr;
    out.trade_cap = parity ? e->cfg.trade_cap : 0;
    e->ntr[b] = e->d_ntr_ring.p + slot;
    out.n_trades = e->ntr[b];
    out.dbg = nullptr;
    if (BT_ABL(e->grid, 64)) {  // profiling stamps (profiling build only)
        e->d_dbg.ensure(kDbgSlots + 8 * kDbgBlocks);
        HIPCHK(hipMemsetAsync(e->d_dbg.p, 0, (kDbgSlots + 8 * kDbgBlocks) * sizeof(unsigned long long), st));
        out.dbg = e->d_dbg.p;
    }
    const bool timing = (e->cfg.flags & BT_FLAG_TIMING) != 0;
    std::pair<Event, Event> ev;  // ours until it reaches ev_pending: a throw before that destroys it
    if (timing) {
        if (!e->ev_pool.empty()) {
            ev = std::move(e->ev_pool.back());
            e->ev_pool.pop_back();
        }
        ev.first.ensure(0);
        ev.second.ensure(0);
        HIPCHK(hipEventRecord(ev.first, st));
    }
    SegArgs sg{nullptr, nullptr, nullptr, nullptr, pl.G, pl.burn_tiles};
    if (pl.G > 1) {
        e->d_seg.ensure(pl.seg_slots);
        sg.rec = e->d_seg.p;
        if (pl.pos_bytes) sg.pos = reinterpret_cast<int8_t*>(e->d_seg.p) + pl.pos_off;
        if (pl.ema_doubles) {
            e->d_segema.ensure(pl.ema_doubles);
            sg.ema = e->d_segema.p;
        }
        e->d_refixed.ensure(1);
        HIPCHK(hipMemsetAsync(e->d_refixed.p, 0, sizeof(unsigned long long), st));
        sg.refixed = e->d_refixed.p;
    }
    e->seg_last = pl.G;
    hipError_t err;
    switch (e->cfg.strategy) {
        case BT_SMA_CROSS:
            err = launch_sma(e->d_syms.p, S, e->d_c.p, e->grid, out, parity, sg, pl, st);
            break;
        case BT_EMA_OLS:
            err = launch_ema_ols(e->d_syms.p, S, e->d_c.p, e->grid, out, parity, sg, pl, st);
            break;
        default:
            err = launch_boll(e->d_syms.p, S, e->d_h.p, e->d_l.p, e->d_c.p, e->grid, out, parity, sg, pl,
                              st);
            break;
    }
    HIPCHK(err);
    // the kernel-done event the top-k chain and, for a run on the run stream, the engine stream's
    // next join wait for: the timing end event when there is one (one marker less between two
    // runs' kernels; it stays recorded until a drained run's pair is handed out again, and a
    // drained run has finished)
    hipEvent_t kdone = e->ev_kdone[on_run];
    if (timing) {
        HIPCHK(hipEventRecord(ev.second, st));
        kdone = ev.second;
        e->ev_pending.push_back(std::move(ev));
    } else if (e->cfg.topk > 0 || on_run) {
        HIPCHK(hipEventRecord(kdone, st));
    }
    if (on_run) e->r_last = kdone;
    if (e->cfg.topk > 0) {
        HIPCHK(hipStreamWaitEvent(e->tstream, kdone, 0));
        HIPCHK(launch_topk(e->d_key[b].p, e->d_sum[b].p, e->d_syms.p, (int64_t)S * e->P, e->P,
                           e->cfg.topk, topk_work(e), e->tstream, pl.topk_lds_free));
        HIPCHK(hipEventRecord(e->ev_tdone[b], e->tstream));
        e->tdone_armed[b] = true;
    }
    e->ran = true;
}

void drain_timing(bt_engine* e) {
    // A run counts from its start or from the end of the run before it, whichever is later: on
    // two streams run i's start event fires while run i-1 still executes, and the start-to-end
    // intervals of a pipelined loop would add up to more than the time its kernels covered. For
    // runs a wait apart both give the start-to-end interval.
    for (auto& ev : e->ev_pending) {
        HIPCHK(hipEventSynchronize(ev.second));
        if (e->r_last == ev.second.ev) e->r_last = nullptr;  // finished: nothing left to join
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, ev.first, ev.second));
        if (e->ev_last.second) {
            float since = 0.f;
            HIPCHK(hipEventElapsedTime(&since, e->ev_last.second, ev.second));
            ms = std::min(ms, std::max(since, 0.f));
            e->ev_pool.push_back(std::move(e->ev_last));
        }
        e->kernel_ms += ms;
        e->launches += 1;
        e->ev_last = std::move(ev);  // its end event stays recorded until the next run is drained
    }
    e->ev_pending.clear();
}


std::vector<bt_topk_rec> read_topk_impl(bt_engine* e, int32_t k) {
    if (!e->ran || e->cfg.topk <= 0) throw HipFail{"top-k not computed (topk == 0 or no run)"};
    // header + the configured k records in one copy into pinned memory
    const size_t nrec = (size_t)e->cfg.topk + 1;
    HIPCHK(hipMemcpyAsync(e->h_top.p, e->d_top.p, nrec * sizeof(bt_topk_rec), hipMemcpyDeviceToHost,
                          e->tstream));
    sync_all(e);
    int32_t n = 0;
    memcpy(&n, e->h_top.p, sizeof n);
    // the device selection is complete whatever the ties (k_topk.hip topk_finish_ties)
    if (n < 0 || n > e->cfg.topk) throw HipFail{"device top-k returned a bad record count"};
    std::vector<bt_topk_rec> res(e->h_top.p + 1, e->h_top.p + 1 + n);
    if ((int32_t)res.size() > k) res.resize(k);
    return res;
}

// The device half of bt_run_batch (step 4 of batch.h's Batch): pinned staging for the host half
// to fill, then one async H2D per column, the strategy kernel, one D2H of every summary, one wait.
void run_batch_impl(bt_engine* e, size_t n, const bt_job_in* jobs, bt_job_out* outs) {
    Batch bat(n, jobs, e->cfg.host_threads);
    activate(e);
    sync_all(e);  // staging and h_sum may still be in use by an earlier call
    const int64_t rows = bat.parse();
    const int ncol = has_hl(e) ? 3 : 1;
    for (int k = 0; k < ncol; ++k) e->h_stage[k].ensure((size_t)rows);
    bat.stage(e->h_stage[0].p, ncol == 3 ? e->h_stage[1].p : nullptr, ncol == 3 ? e->h_stage[2].p : nullptr);
    bt_batch_profile& pr = bat.prof;
    e->n_errors = pr.n_failed;
    const size_t nres = bat.syms.size() * (size_t)e->P;
    if (!bat.syms.empty()) {
        std::vector<SymDesc> syms;
        for (const StagedSym& s : bat.syms) syms.push_back(SymDesc{s.row, s.bars, (int32_t)syms.size()});
        for (Event& ev : e->ev_batch) ev.ensure(0);
        e->h_sum.ensure(nres);
        set_dataset(e, std::move(syms), rows);
        HIPCHK(hipEventRecord(e->ev_batch[0], main_stream(e)));
        int32_t* dst[3] = {e->d_c.p, e->d_h.p, e->d_l.p};
        for (int k = 0; k < ncol; ++k)
            HIPCHK(hipMemcpyAsync(dst[k], e->h_stage[k].p, (size_t)rows * 4, hipMemcpyHostToDevice,
                                  main_stream(e)));
        HIPCHK(hipEventRecord(e->ev_batch[1], main_stream(e)));
        run_impl(e);
        HIPCHK(hipEventRecord(e->ev_batch[2], main_stream(e)));
        HIPCHK(hipMemcpyAsync(e->h_sum.p, e->d_sum[e->cur].p, nres * sizeof(bt_summary),
                              hipMemcpyDeviceToHost, main_stream(e)));
        HIPCHK(hipEventRecord(e->ev_batch[3], main_stream(e)));
        sync_all(e);
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e->ev_batch[0], e->ev_batch[1]));
        pr.upload_ms = ms;
        HIPCHK(hipEventElapsedTime(&ms, e->ev_batch[1], e->ev_batch[2]));
        pr.compute_ms = ms;
        HIPCHK(hipEventElapsedTime(&ms, e->ev_batch[2], e->ev_batch[3]));
        pr.readback_ms = ms;
    }
    bat.format(e->h_sum.p, e->P, outs);
    e->prof = pr;
}

}  // namespace

// Device sources of the multi-GPU exchange (comm.cpp): the last run's top-k (header record +
// records) and trade counter, on the engine's top-k stream after the run's top-k chain.
bool bt::engine_exchange_view(bt_engine* e, ExchangeView& v, std::string& err) {
    if (!e || !e->ran || e->cfg.topk <= 0 || !e->d_top.p) {
        err = "exchange needs an engine with topk > 0 and a finished bt_run";
        return false;
    }
    v.tstream = e->tstream;
    v.device = e->cfg.device;
    v.topk = e->cfg.topk;
    v.d_top = e->d_top.p;
    v.d_ntr = e->ntr[e->cur];
    v.bar_evals = 0;
    for (const SymDesc& s : e->syms) v.bar_evals += (int64_t)s.bars * e->P;
    return true;
}

// The exchange's copies out of the run's buffers were enqueued on tstream: the next run that
// reuses those buffers waits for them (same bookkeeping as bt_topk_fetch_async).
void bt::engine_exchange_enqueued(bt_engine* e) {
    if (hipEventRecord(e->ev_tdone[e->cur], e->tstream) == hipSuccess) e->tdone_armed[e->cur] = true;
}

extern "C" {

int32_t bt_abi_version(void) { return BT_ABI_VERSION; }

const char* bt_last_error(void) { return g_err.c_str(); }

static bt_engine* create_impl(const bt_config* cfg) {
    if (cfg == nullptr) throw HipFail{"null config"};
    auto e = std::make_unique<bt_engine>();  // a failure below frees what was made so far
    e->cfg = *cfg;
    const std::string m = validate_and_copy(e.get(), *cfg);
    if (!m.empty()) throw HipFail{m};
    e->cfg.fast = e->cfg.slow = e->cfg.span = e->cfg.ols = nullptr;
    e->cfg.bwin = e->cfg.k_num = e->cfg.sl_bps = e->cfg.tp_bps = nullptr;
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (cfg->device < 0 || cfg->device >= ndev)
        throw HipFail{"HIP device " + std::to_string(cfg->device) + " not present (" +
                      std::to_string(ndev) + " visible)"};
    activate(e.get());
    if (hipDeviceGetAttribute(&e->cus, hipDeviceAttributeMultiprocessorCount, cfg->device) != hipSuccess ||
        e->cus <= 0)
        e->cus = kCusFallback;
    if (cfg->stream)
        e->stream.borrow((hipStream_t)cfg->stream);
    else
        e->stream.create();
    if (e->stream.owned) e->rstream.create();
    e->tstream.create();
    for (Event& ev : e->ev_kdone) ev.ensure(hipEventDisableTiming);
    e->ev_main.ensure(hipEventDisableTiming);
    for (Event& ev : e->ev_tdone) ev.ensure(hipEventDisableTiming);
    upload_grid(e.get());
#ifdef BT_PROFILING
    if (const char* ab = getenv("BT_ABLATE")) e->grid.ablate = atoi(ab);  // profiling build only
#endif
    return e.release();
}

bt_engine* bt_engine_create(const bt_config* cfg, char* err, size_t errlen) {
    auto failed = [&]() -> bt_engine* {  // bt_last_error() into the caller's buffer too
        if (err && errlen) snprintf(err, errlen, "%s", g_err.c_str());
        return nullptr;
    };
    ABI_GUARD(failed(), { return create_impl(cfg); })
}

void bt_engine_destroy(bt_engine* e) {
    if (!e) return;
    try {
        delete e;
    } catch (...) {
    }
}

int32_t bt_num_params(const bt_engine* e) { return e ? e->P : -1; }

int32_t bt_set_segments(bt_engine* e, int32_t segments, int32_t burn_tiles) {
    ABI_GUARD(-1, {
        if (!e || segments < 0 || segments > 64 || burn_tiles < 0) throw HipFail{"bad arguments"};
        e->seg_req = segments;
        e->burn_req = burn_tiles;
        return 0;
    })
}

int32_t bt_set_run_overlap(bt_engine* e, int32_t on) {
    ABI_GUARD(-1, {
        if (!e) throw HipFail{"bt_set_run_overlap: null engine"};
        e->overlap_on = on != 0;  // the planner reads it per run; any mix of runs stays ordered
        return 0;
    })
}

int32_t bt_last_segments(bt_engine* e, int64_t* refixed_blocks) {
    ABI_GUARD(-1, {
        if (!e) throw HipFail{"null engine"};
        if (refixed_blocks) {
            unsigned long long n = 0;
            if (e->seg_last > 1 && e->d_refixed.p) {
                activate(e);
                sync_all(e);
                HIPCHK(hipMemcpy(&n, e->d_refixed.p, sizeof n, hipMemcpyDeviceToHost));
            }
            *refixed_blocks = (int64_t)n;
        }
        return e->seg_last;
    })
}

int32_t bt_load_synthetic(bt_engine* e, uint64_t seed, int64_t sym_begin, int32_t n_sym,
                          int32_t n_bars, int32_t freq) {
    ABI_GUARD(-1, {
        if (!e) throw HipFail{"null engine"};
        if (n_sym < 0 || n_bars < 1 || n_bars > kMaxBars) throw HipFail{"bad synthetic shape"};
        if (sym_begin < 0 || sym_begin + n_sym > (1LL << 31)) throw HipFail{"bad symbol ids"};
        if (freq != BT_DAILY && freq != BT_MINUTE) throw HipFail{"bad freq"};
        activate(e);
        std::vector<int32_t> bars(n_sym, n_bars);
        std::vector<int64_t> ids(n_sym);
        for (int32_t s = 0; s < n_sym; ++s) ids[s] = sym_begin + s;
        layout(e, n_sym, bars.data(), ids.data());
        HIPCHK(launch_gen(e->d_syms.p, n_sym, seed, freq, nullptr, has_hl(e) ? e->d_h.p : nullptr,
                          has_hl(e) ? e->d_l.p : nullptr, e->d_c.p, main_stream(e)));
        sync_all(e);
        return 0;
    })
}

int32_t bt_load_ohlc(bt_engine* e, int32_t n_sym, const int64_t* sym_ids, const int32_t* bars,
                     const int64_t* row_off, const int32_t* h, const int32_t* l, const int32_t* c) {
    ABI_GUARD(-1, {
        if (!e || n_sym < 0 || (n_sym > 0 && (!sym_ids || !bars || !row_off || !c)))
            throw HipFail{"bad arguments"};
        if (has_hl(e) && (!h || !l)) throw HipFail{"strategy needs high and low columns"};
        for (int32_t s = 0; s < n_sym; ++s)
            if (bars[s] < 1 || bars[s] > kMaxBars) throw HipFail{"bad bar count"};
        // the id rule (topk_rules.h), before anything is laid out: a refused call leaves the
        // resident dataset as it was
        const std::string bad_id = sym_id_refusal(n_sym, sym_ids);
        if (!bad_id.empty()) throw HipFail{"bt_load_ohlc: " + bad_id};
        activate(e);
        sync_all(e);  // the pinned staging may still feed an earlier upload
        layout(e, n_sym, bars, sym_ids);
        // stage into pinned host rows with the device row layout, then one async copy per
        // column and a single wait
        const int ncol = has_hl(e) ? 3 : 1;
        const int32_t* src[3] = {c, h, l};
        int32_t* dst[3] = {e->d_c.p, e->d_h.p, e->d_l.p};
        if (e->rows > 0) {
            for (int k = 0; k < ncol; ++k) {
                e->h_stage[k].ensure((size_t)e->rows);
                for (int32_t s = 0; s < n_sym; ++s)
                    memcpy(e->h_stage[k].p + e->syms[s].off, src[k] + row_off[s], (size_t)bars[s] * 4);
                HIPCHK(hipMemcpyAsync(dst[k], e->h_stage[k].p, (size_t)e->rows * 4,
                                      hipMemcpyHostToDevice, main_stream(e)));
            }
            sync_all(e);
        }
        return 0;
    })
}

int32_t bt_run(bt_engine* e) {
    ABI_GUARD(-1, {
        if (!e) throw HipFail{"null engine"};
        run_impl(e);
        return 0;
    })
}

int32_t bt_sync(bt_engine* e) {
    ABI_GUARD(-1, {
        if (!e) throw HipFail{"null engine"};
        activate(e);
        sync_all(e);
        return 0;
    })
}

int32_t bt_read_summaries(bt_engine* e, bt_summary* out, size_t n) {
    ABI_GUARD(-1, {
        if (!e || !e->ran) throw HipFail{"no results"};
        const size_t have = e->syms.size() * (size_t)e->P;
        if (n > have) throw HipFail{"n exceeds symbols x params"};
        activate(e);
        sync_all(e);
        HIPCHK(hipMemcpy(out, e->d_sum[e->cur].p, n * sizeof(bt_summary), hipMemcpyDeviceToHost));
        return 0;
    })
}

int32_t bt_read_sums(bt_engine* e, bt_sums* out, size_t n) {
    ABI_GUARD(-1, {
        if (!e || !e->ran || !(e->cfg.flags & BT_FLAG_PARITY)) throw HipFail{"no parity results"};
        if (n > e->syms.size() * (size_t)e->P) throw HipFail{"n too large"};
        activate(e);
        sync_all(e);
        HIPCHK(hipMemcpy(out, e->d_sums.p, n * sizeof(bt_sums), hipMemcpyDeviceToHost));
        return 0;
    })
}

int32_t bt_read_trades(bt_engine* e, bt_trade* out, size_t n) {
    ABI_GUARD(-1, {
        if (!e || !e->ran || !(e->cfg.flags & BT_FLAG_PARITY)) throw HipFail{"no parity results"};
        if (n > e->syms.size() * (size_t)e->P * e->cfg.trade_cap) throw HipFail{"n too large"};
        activate(e);
        sync_all(e);
        HIPCHK(hipMemcpy(out, e->d_trades.p, n * sizeof(bt_trade), hipMemcpyDeviceToHost));
        return 0;
    })
}

int32_t bt_read_topk(bt_engine* e, bt_topk_rec* out, int32_t k) {
    ABI_GUARD(-1, {
        if (!e || !out || k <= 0) throw HipFail{"bad arguments"};
        activate(e);
        std::vector<bt_topk_rec> r = read_topk_impl(e, std::min(k, e->cfg.topk));
        std::copy(r.begin(), r.end(), out);
        return (int32_t)r.size();
    })
}

int32_t bt_topk_fetch_async(bt_engine* e, int32_t slot) {
    ABI_GUARD(-1, {
        if (!e || slot < 0 || slot >= BT_PIPE_SLOTS) throw HipFail{"bad arguments"};
        if (!e->ran || e->cfg.topk <= 0) throw HipFail{"top-k not computed (topk == 0 or no run)"};
        activate(e);
        e->h_slot[slot].ensure(kTopkMax + 2);
        e->slot_ev[slot].ensure(hipEventDisableTiming);
        bt_topk_rec* h = e->h_slot[slot].p;
        // behind the run's top-k chain on tstream; the trade counter of the run's buffer is
        // complete too (the chain waited for the kernel)
        HIPCHK(hipMemcpyAsync(h, e->d_top.p, ((size_t)e->cfg.topk + 1) * sizeof(bt_topk_rec),
                              hipMemcpyDeviceToHost, e->tstream));
        HIPCHK(hipMemcpyAsync(h + kTopkMax + 1, e->ntr[e->cur], sizeof(unsigned long long),
                              hipMemcpyDeviceToHost, e->tstream));
        HIPCHK(hipEventRecord(e->slot_ev[slot], e->tstream));
        HIPCHK(hipEventRecord(e->ev_tdone[e->cur], e->tstream));  // buffer readers now end here
        e->slot_armed[slot] = true;
        return 0;
    })
}

int32_t bt_topk_fetch_wait(bt_engine* e, int32_t slot, bt_topk_rec* out, int32_t k,
                           int64_t* n_trades) {
    ABI_GUARD(-1, {
        if (!e || slot < 0 || slot >= BT_PIPE_SLOTS || !out || k <= 0) throw HipFail{"bad arguments"};
        if (!e->slot_armed[slot]) throw HipFail{"no fetch pending on this slot"};
        activate(e);
        HIPCHK(hipEventSynchronize(e->slot_ev[slot]));
        const bt_topk_rec* h = e->h_slot[slot].p;
        int32_t n = 0;
        memcpy(&n, h, sizeof n);
        if (n < 0 || n > e->cfg.topk) throw HipFail{"device top-k returned a bad record count"};
        const int32_t m = std::min(n, std::min(k, e->cfg.topk));
        std::copy(h + 1, h + 1 + m, out);
        if (n_trades) {
            unsigned long long t = 0;
            memcpy(&t, h + kTopkMax + 1, sizeof t);
            *n_trades = (int64_t)t;
        }
        return m;
    })
}

int32_t bt_read_stats(bt_engine* e, bt_stats* out) {
    ABI_GUARD(-1, {
        if (!e || !out) throw HipFail{"bad arguments"};
        activate(e);
        sync_all(e);
        bt_stats st{};
        st.n_symbols = (int64_t)e->syms.size();
        st.n_params = e->P;
        for (const SymDesc& s : e->syms) st.bar_evals += (int64_t)s.bars * e->P;
        st.errors = e->n_errors;
        if (e->ran) {
            unsigned long long n = 0;
            HIPCHK(hipMemcpy(&n, e->ntr[e->cur], sizeof n, hipMemcpyDeviceToHost));
            st.trades = (int64_t)n;
        }
        *out = st;
        return 0;
    })
}

int32_t bt_read_close(bt_engine* e, int32_t sym_index, int32_t* out, int32_t n) {
    ABI_GUARD(-1, {
        if (!e || sym_index < 0 || sym_index >= (int32_t)e->syms.size()) throw HipFail{"bad symbol"};
        const SymDesc& sd = e->syms[sym_index];
        if (n > sd.bars) throw HipFail{"n exceeds bars"};
        activate(e);
        sync_all(e);
        HIPCHK(hipMemcpy(out, e->d_c.p + sd.off, (size_t)n * 4, hipMemcpyDeviceToHost));
        return 0;
    })
}

int32_t bt_read_debug(bt_engine* e, uint64_t* out, int32_t n) {
    ABI_GUARD(-1, {
        if (!e || !out || n < 0 || n > kDbgSlots + 8 * kDbgBlocks || !e->d_dbg.p) throw HipFail{"no debug stamps"};
        activate(e);
        sync_all(e);
        HIPCHK(hipMemcpy(out, e->d_dbg.p, (size_t)n * 8, hipMemcpyDeviceToHost));
        return 0;
    })
}

int32_t bt_kernel_timing(bt_engine* e, double* total_ms, int64_t* launches, const char** name) {
    ABI_GUARD(-1, {
        if (!e) throw HipFail{"null engine"};
        activate(e);
        drain_timing(e);
        if (total_ms) *total_ms = e->kernel_ms;
        if (launches) *launches = e->launches;
        if (name) *name = kernel_name(e->cfg.strategy);
        return 0;
    })
}

int32_t bt_reset_timing(bt_engine* e) {
    ABI_GUARD(-1, {
        if (!e) throw HipFail{"null engine"};
        activate(e);
        drain_timing(e);
        e->kernel_ms = 0.0;
        e->launches = 0;
        return 0;
    })
}

int32_t bt_run_batch(bt_engine* e, size_t n, const bt_job_in* jobs, bt_job_out* outs) {
    ABI_GUARD(-1, {
        if (!e || (n > 0 && (!jobs || !outs))) throw HipFail{"bad arguments"};
        for (size_t i = 0; i < n; ++i) outs[i] = bt_job_out{nullptr, 0, 0, 0};
        try {
            run_batch_impl(e, n, jobs, outs);
        } catch (...) {
            bt_job_out_free(outs, n);  // a failed call leaves no string allocated
            throw;
        }
        return 0;
    })
}

int32_t bt_last_batch_profile(bt_engine* e, bt_batch_profile* out) {
    ABI_GUARD(-1, {
        if (!e || !out) throw HipFail{"bad arguments"};
        *out = e->prof;
        return 0;
    })
}

int64_t bt_format_summaries(const bt_summary* r, int32_t P, char* out, size_t cap) {
    ABI_GUARD(-1, {
        if (P < 0) throw HipFail{"bad arguments"};
        if (!out) return (int64_t)((size_t)P * kLineMax);
        if (P > 0 && !r) throw HipFail{"bad arguments"};
        if (cap < (size_t)P * kLineMax) throw HipFail{"output buffer too small"};
        return (int64_t)fmt_job_into(r, P, out);
    })
}

void bt_job_out_free(bt_job_out* outs, size_t n) {
    if (outs) free_job_outs(outs, n);
}

int32_t bt_merge_topk(const bt_topk_rec* in, size_t n, int32_t k, bt_topk_rec* out) {
    ABI_GUARD(-1, {
        if ((n > 0 && !in) || !out || k < 0) throw HipFail{"bad arguments"};
        std::vector<bt_topk_rec> v(in, in + n);
        std::sort(v.begin(), v.end(), topk_less);
        const size_t m = std::min<size_t>(v.size(), (size_t)k);
        std::copy(v.begin(), v.begin() + m, out);
        return (int32_t)m;
    })
}

double bt_i128_to_double(uint64_t lo, int64_t hi) { return i128_to_double(lo, hi); }

int32_t bt_parse_csv(const uint8_t* buf, size_t len, int32_t cap, int32_t* h, int32_t* l,
                     int32_t* c, char* err, size_t errlen) {
    return bt_parse_job(buf, len, cap, h, l, c, err, errlen);
}

int64_t bt_encode_columns(const int32_t* o, const int32_t* h, const int32_t* l, const int32_t* c,
                          const int64_t* v, int32_t n, uint8_t* out, size_t cap) {
    ABI_GUARD(-1, {
        if (n < 1 || n > kMaxBars || !o || !h || !l || !c) throw HipFail{"bad arguments"};
        const size_t need = binary_payload_size(n, v != nullptr);
        if (!out) return (int64_t)need;
        if (cap < need) throw HipFail{"output buffer too small"};
        return (int64_t)encode_binary(o, h, l, c, v, n, out);
    })
}

int64_t bt_gen_payload(uint64_t seed, int64_t sym, int32_t bars, int32_t freq, uint8_t* out,
                       size_t cap) {
    ABI_GUARD(-1, {
        if (bars < 1 || bars > kMaxBars || (freq != BT_DAILY && freq != BT_MINUTE))
            throw HipFail{"bad arguments"};
        const size_t need = binary_payload_size(bars, true);
        if (!out) return (int64_t)need;
        if (cap < need) throw HipFail{"output buffer too small"};
        std::vector<int32_t> o((size_t)bars), h((size_t)bars), l((size_t)bars), c((size_t)bars);
        std::vector<int64_t> v((size_t)bars);
        gen_host(seed, sym, bars, freq, o.data(), h.data(), l.data(), c.data(), v.data());
        return (int64_t)encode_binary(o.data(), h.data(), l.data(), c.data(), v.data(), bars, out);
    })
}

int32_t bt_parse_job(const uint8_t* buf, size_t len, int32_t cap, int32_t* h, int32_t* l,
                     int32_t* c, char* err, size_t errlen) {
    ABI_GUARD(-1, {
        Bars b;
        std::string m;
        if (!parse_job(buf, len, b, m)) {
            if (err && errlen) snprintf(err, errlen, "%s", m.c_str());
            set_last_error(m);
            return -1;
        }
        if ((int64_t)b.c.size() > cap) throw HipFail{"cap too small"};
        if (h) memcpy(h, b.h.data(), b.h.size() * 4);
        if (l) memcpy(l, b.l.data(), b.l.size() * 4);
        if (c) memcpy(c, b.c.data(), b.c.size() * 4);
        return (int32_t)b.c.size();
    })
}

}  // extern "C"
