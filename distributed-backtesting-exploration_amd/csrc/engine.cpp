// engine.cpp — the C ABI of include/bt.h: engine lifecycle, HBM-resident datasets, the
// JobsReply batch entry point (drop-in for process_incoming_job,
// /root/reference/src/worker/process.rs:13-29); its host half, ingest and result strings, is batch.cpp.
//
// Nothing here computes a backtest on the CPU: every result comes from the HIP kernels in
// k_*.hip. The host moves bars to HBM, launches and reads back; the HIP objects it holds are the
// self-freeing types of hip_owned.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "batch.h"
#include "csv.h"
#include "hip_owned.h"
#include "internal.h"
#include "plan.h"
#include "surface.h"
#include "walkfwd.h"

using namespace bt;

static thread_local std::string g_err;

void bt::set_last_error(const std::string& s) { g_err = s; }

constexpr int64_t kNtrRing = 64;  // per-run trade counter slots (bt_engine::d_ntr_ring)

struct bt_engine {
    bt_config cfg{};
    std::vector<int32_t> ax[4];  // owned copies of the grid axes
    Grid grid{};
    int32_t P = 0;
    // the engine stream (its own, or bt_config.stream borrowed) and the top-k chain stream (the
    // chain of run i overlaps the kernel of run i+1). Declared before every buffer and event:
    // members go in reverse order, so the streams outlive what was enqueued on them
    Stream tstream, stream;
    // What is still enqueued finishes before the members free what it uses. The engine stream is
    // the first HIP object an engine makes: without it there is nothing to wait for.
    ~bt_engine() {
        if (!stream) return;
        (void)hipSetDevice(cfg.device);
        (void)hipStreamSynchronize(stream);
        if (tstream) (void)hipStreamSynchronize(tstream);
    }
    DevBuf<int32_t> d_axes[4];
    DevBuf<int32_t> d_kwin;      // SMA: Grid::kwin, Grid::krecip
    DevBuf<double> d_krecip;
    // dataset
    std::vector<SymDesc> syms;
    int64_t rows = 0;
    DevBuf<SymDesc> d_syms;
    DevBuf<int32_t> d_c, d_h, d_l;
    // outputs, double-buffered: run i writes buffer i % 2 while the top-k chain of run i-1
    // (on tstream) still reads the other one; `cur` is the buffer of the last run
    DevBuf<bt_summary> d_sum[2];
    DevBuf<uint64_t> d_key[2];
    // per-run trade counters: a ring of kNtrRing slots, run r accumulating into slot
    // r % kNtrRing; half the ring is zeroed every kNtrRing / 2 runs (slots last used >= 33 runs
    // earlier), so a run enqueues no memset of its own. ntr[b]: the slot of the last run that
    // wrote output buffer b
    DevBuf<unsigned long long> d_ntr_ring;
    unsigned long long* ntr[2] = {nullptr, nullptr};
    int cur = 0;
    int64_t nrun = 0;
    DevBuf<bt_sums> d_sums;
    DevBuf<bt_trade> d_trades;
    int cus = kCusFallback;      // compute units of the device (launch plans, plan.h)
    int32_t max_bars = 0;        // bars of the longest symbol
    // bar segments: requested count (0 = auto, 1 = off) and burn-in tiles (0 = the strategy's
    // default), the records of a split run and the count the last run used
    int32_t seg_req = 0, burn_req = 0, seg_last = 1;
    DevBuf<SegRec> d_seg;
    DevBuf<double> d_segema;
    DevBuf<unsigned long long> d_refixed;
    DevBuf<unsigned long long> d_dbg;
    Event ev_kdone;      // kernel of the last run finished (main stream)
    Event ev_tdone[2];   // readers of buffer b finished (tstream)
    bool tdone_armed[2] = {false, false};
    // top-k work
    DevBuf<unsigned int> d_hist, d_counts;
    DevBuf<unsigned long long> d_state, d_above, d_cand;
    DevBuf<bt_topk_rec> d_top;
    PinnedBuf<bt_topk_rec> h_top;     // pinned host copy of d_top
    // pipelined read-back slots: header + kTopkMax records + one record holding the trade count
    PinnedBuf<bt_topk_rec> h_slot[BT_PIPE_SLOTS];
    Event slot_ev[BT_PIPE_SLOTS];
    bool slot_armed[BT_PIPE_SLOTS] = {};
    bool topk_ready = false;          // top-k buffers allocated and their state initialised
    bool ran = false;
    // timing of the dominant kernel
    std::vector<std::pair<Event, Event>> ev_pending, ev_pool;
    double kernel_ms = 0.0;
    int64_t launches = 0;
    // bt_run_batch: pinned host staging of the columns in device row layout (c, h, l), the
    // batch's summaries read back in one copy, phase events and the last batch's profile
    PinnedBuf<int32_t> h_stage[3];
    PinnedBuf<bt_summary> h_sum;
    Event ev_batch[4];
    bt_batch_profile prof{};
    int64_t n_errors = 0;
    // bt_replay: device staging of one chunk of requests (descriptors, summaries, trades, curves),
    // at most kReplayBudget bytes whatever n and stride are
    DevBuf<uint8_t> d_replay;
    // bt_surface: requested row chunks (0 = the planner's choice), the partials and results of
    // one reduction, and the matrix and ids bt_surface_of stages
    int32_t surface_chunks = 0;
    DevBuf<uint8_t> d_surface, d_surface_in;
    PinnedBuf<uint8_t> h_surface;  // the results of one reduction
    // bt_walk_forward: the staging budget asked for (0 = kWalkfwdBudget) and the device staging
    // of one chunk of rows (bounds, fold records, steps), never more than the budget
    int64_t walkfwd_budget = 0;
    DevBuf<uint8_t> d_walkfwd;
};

namespace {

void activate(bt_engine* e) { HIPCHK(hipSetDevice(e->cfg.device)); }

bool has_hl(const bt_engine* e) { return e->cfg.strategy == BT_BOLL; }

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

void sync_all(bt_engine* e);

// Install a dataset: symbol descriptors (row offsets into the columns) and `rows` rows per
// column; allocates the columns the strategy needs.
void set_dataset(bt_engine* e, std::vector<SymDesc>&& syms, int64_t rows) {
    // the previous run's top-k chain (second stream) reads the symbol descriptors (ids of its
    // records), and a column may be reallocated below: both streams drain first (the upload on
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
                              hipMemcpyHostToDevice, e->stream));
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

void sync_all(bt_engine* e) {
    HIPCHK(hipStreamSynchronize(e->stream));
    if (e->tstream) HIPCHK(hipStreamSynchronize(e->tstream));
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
        HIPCHK(launch_topk_init(topk_work(e), e->stream));
        e->topk_ready = true;
    }
}

void run_impl(bt_engine* e) {
    activate(e);
    ensure_outputs(e);
    const int32_t S = (int32_t)e->syms.size();
    const int64_t run = e->nrun++;
    const int b = (int)(run & 1);
    e->cur = b;
    // buffer b was last read by the top-k chain / read-back of run i-2: wait for them (no wait
    // packet when they have already finished, the steady state of a pipelined sweep)
    if (e->tdone_armed[b] && hipEventQuery(e->ev_tdone[b]) != hipSuccess)
        HIPCHK(hipStreamWaitEvent(e->stream, e->ev_tdone[b], 0));
    Out out{};
    out.sum = e->d_sum[b].p;
    out.key = e->d_key[b].p;
    const bool parity = (e->cfg.flags & BT_FLAG_PARITY) != 0;
    out.sums = parity ? e->d_sums.p : nullptr;
    out.trades = parity ? e->d_trades.p : nullptr;
    out.trade_cap = parity ? e->cfg.trade_cap : 0;
    const int slot = (int)(run % kNtrRing);
    if (slot % (kNtrRing / 2) == 0)
        HIPCHK(hipMemsetAsync(e->d_ntr_ring.p + slot, 0, (kNtrRing / 2) * sizeof(unsigned long long),
                              e->stream));
    e->ntr[b] = e->d_ntr_ring.p + slot;
    out.n_trades = e->ntr[b];
    out.dbg = nullptr;
    if (BT_ABL(e->grid, 64)) {  // profiling stamps (profiling build only)
        e->d_dbg.ensure(kDbgSlots + 8 * kDbgBlocks);
        HIPCHK(hipMemsetAsync(e->d_dbg.p, 0, (kDbgSlots + 8 * kDbgBlocks) * sizeof(unsigned long long),
                              e->stream));
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
        HIPCHK(hipEventRecord(ev.first, e->stream));
    }
    const LaunchPlan pl = plan_launch(e->grid, e->ax[0].data(),
                                      RunShape{S, e->max_bars, parity, e->seg_req, e->burn_req, e->cus});
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
        HIPCHK(hipMemsetAsync(e->d_refixed.p, 0, sizeof(unsigned long long), e->stream));
        sg.refixed = e->d_refixed.p;
    }
    e->seg_last = pl.G;
    hipError_t err;
    switch (e->cfg.strategy) {
        case BT_SMA_CROSS:
            err = launch_sma(e->d_syms.p, S, e->d_c.p, e->grid, out, parity, sg, pl, e->stream);
            break;
        case BT_EMA_OLS:
            err = launch_ema_ols(e->d_syms.p, S, e->d_c.p, e->grid, out, parity, sg, pl, e->stream);
            break;
        default:
            err = launch_boll(e->d_syms.p, S, e->d_h.p, e->d_l.p, e->d_c.p, e->grid, out, parity, sg, pl,
                              e->stream);
            break;
    }
    HIPCHK(err);
    hipEvent_t kdone = e->ev_kdone;
    if (timing) {
        HIPCHK(hipEventRecord(ev.second, e->stream));
        kdone = ev.second;
        e->ev_pending.push_back(std::move(ev));
    }
    if (e->cfg.topk > 0) {
        // the chain waits for the kernel: on the timing end event when there is one (one
        // marker less between two runs' kernels)
        if (!timing) HIPCHK(hipEventRecord(kdone, e->stream));
        HIPCHK(hipStreamWaitEvent(e->tstream, kdone, 0));
        HIPCHK(launch_topk(e->d_key[b].p, e->d_sum[b].p, e->d_syms.p, (int64_t)S * e->P, e->P,
                           e->cfg.topk, topk_work(e), e->tstream, pl.topk_lds_free));
        HIPCHK(hipEventRecord(e->ev_tdone[b], e->tstream));
        e->tdone_armed[b] = true;
    }
    e->ran = true;
}

// ---- bt_replay: chosen lanes again, with their trades and curves (k_replay.hip)
// Device staging per call is bounded by this budget: the requests are processed in chunks of as
// many lanes as fit (one lane of the longest symbol, 2^22 bars, with its curves and a full trade
// list needs 37.7 + 134 MB, so one lane always fits).
constexpr size_t kReplayBudget = 256u << 20;

int32_t replay_impl(bt_engine* e, int32_t n, const bt_lane* lanes, int32_t trade_cap, bt_summary* sum,
                    int32_t* n_bars, bt_trade* trades, int64_t* equity, int8_t* pos, int64_t stride) {
    auto refuse = [](const std::string& m) { throw HipFail{"bt_replay: " + m}; };
    if (!e) refuse("null engine");
    if (e->syms.empty()) refuse("no dataset loaded");
    if (n < 0 || n > BT_REPLAY_MAX)
        refuse("n = " + std::to_string(n) + " outside [0, " + std::to_string(BT_REPLAY_MAX) + "]");
    if (trade_cap < 0) refuse("trade_cap = " + std::to_string(trade_cap) + " is negative");
    if (trades && trade_cap == 0) refuse("trades given with trade_cap = 0");
    if (!trades && trade_cap > 0)
        refuse("trade_cap = " + std::to_string(trade_cap) + " without a trades buffer");
    if (n == 0) return 0;
    if (!lanes || !sum) refuse("lanes and sum are required");
    // global symbol id -> row; the first row of a repeated id wins
    std::unordered_map<int32_t, int32_t> row;
    row.reserve(e->syms.size());
    for (size_t s = 0; s < e->syms.size(); ++s) row.emplace(e->syms[s].id, (int32_t)s);
    std::vector<ReplayLane> req((size_t)n);
    int32_t W = 0;  // the longest requested symbol
    for (int32_t i = 0; i < n; ++i) {
        const auto it = row.find(lanes[i].sym);
        if (it == row.end())
            refuse("unknown symbol id " + std::to_string(lanes[i].sym) + " (lane " + std::to_string(i) + ")");
        if (lanes[i].param < 0 || lanes[i].param >= e->P)
            refuse("param " + std::to_string(lanes[i].param) + " outside [0, " + std::to_string(e->P) +
                   ") (lane " + std::to_string(i) + ")");
        const SymDesc& sd = e->syms[(size_t)it->second];
        req[i] = ReplayLane{sd.off, sd.bars, lanes[i].param};
        W = std::max(W, sd.bars);
    }
    const bool curves = equity || pos;
    if (curves && stride < W)
        refuse("stride = " + std::to_string(stride) + " shorter than the longest requested symbol (" +
               std::to_string(W) + " bars)");
    activate(e);
    sync_all(e);
    // a lane closes at most one trade per bar: the device rows never need more than W slots
    const int64_t dcap = std::min<int64_t>(trade_cap, W);
    const int64_t pitch = curves ? std::min<int64_t>(stride, align_rows(W)) : 0;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t per_lane = sizeof(ReplayLane) + sizeof(bt_summary) + (size_t)dcap * sizeof(bt_trade) +
                            (equity ? (size_t)pitch * 8 : 0) + (pos ? (size_t)pitch : 0);
    const size_t chunk = std::min<size_t>((size_t)n, std::max<size_t>(1, (kReplayBudget - 5 * 256) / per_lane));
    const size_t o_lane = 0, o_sum = up(chunk * sizeof(ReplayLane));
    const size_t o_tr = o_sum + up(chunk * sizeof(bt_summary));
    const size_t o_eq = o_tr + up(chunk * (size_t)dcap * sizeof(bt_trade));
    const size_t o_pos = o_eq + (equity ? up(chunk * (size_t)pitch * 8) : 0);
    const size_t total = o_pos + (pos ? up(chunk * (size_t)pitch) : 0);
    e->d_replay.ensure(total);
    uint8_t* base = e->d_replay.p;
    ReplayOut out{};
    out.sum = reinterpret_cast<bt_summary*>(base + o_sum);
    out.trades = dcap ? reinterpret_cast<bt_trade*>(base + o_tr) : nullptr;
    out.trade_cap = (int32_t)dcap;
    out.equity = equity ? reinterpret_cast<int64_t*>(base + o_eq) : nullptr;
    out.pos = pos ? reinterpret_cast<int8_t*>(base + o_pos) : nullptr;
    out.pitch = pitch;
    // rows of a host array -> rows of a device one: one copy when the pitches agree, else a 2-D
    // copy and the host tails zeroed here
    auto fetch = [&](void* dst, size_t dst_pitch, const void* src, size_t src_pitch, size_t m) {
        if (dst_pitch == src_pitch) {
            HIPCHK(hipMemcpyAsync(dst, src, m * src_pitch, hipMemcpyDeviceToHost, e->stream));
            return;
        }
        HIPCHK(hipMemcpy2DAsync(dst, dst_pitch, src, src_pitch, src_pitch, m, hipMemcpyDeviceToHost, e->stream));
        for (size_t i = 0; i < m; ++i)
            memset(static_cast<uint8_t*>(dst) + i * dst_pitch + src_pitch, 0, dst_pitch - src_pitch);
    };
    for (size_t i0 = 0; i0 < (size_t)n; i0 += chunk) {
        const size_t m = std::min(chunk, (size_t)n - i0);
        HIPCHK(hipMemcpyAsync(base + o_lane, req.data() + i0, m * sizeof(ReplayLane), hipMemcpyHostToDevice, e->stream));
        if (dcap) HIPCHK(hipMemsetAsync(base + o_tr, 0, m * (size_t)dcap * sizeof(bt_trade), e->stream));
        if (equity) HIPCHK(hipMemsetAsync(base + o_eq, 0, m * (size_t)pitch * 8, e->stream));
        if (pos) HIPCHK(hipMemsetAsync(base + o_pos, 0, m * (size_t)pitch, e->stream));
        HIPCHK(launch_replay(reinterpret_cast<const ReplayLane*>(base + o_lane), (int32_t)m, e->d_h.p, e->d_l.p,
                             e->d_c.p, e->grid, out, e->stream));
        HIPCHK(hipMemcpyAsync(sum + i0, out.sum, m * sizeof(bt_summary), hipMemcpyDeviceToHost, e->stream));
        if (dcap)
            fetch(trades + i0 * (size_t)trade_cap, (size_t)trade_cap * sizeof(bt_trade), out.trades,
                  (size_t)dcap * sizeof(bt_trade), m);
        if (equity) fetch(equity + i0 * (size_t)stride, (size_t)stride * 8, out.equity, (size_t)pitch * 8, m);
        if (pos) fetch(pos + i0 * (size_t)stride, (size_t)stride, out.pos, (size_t)pitch, m);
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    if (n_bars)
        for (int32_t i = 0; i < n; ++i) n_bars[i] = req[i].bars;
    return n;
}

// ---- bt_surface / bt_surface_of: the run's summaries reduced on the device (k_surface.hip)
// `d_sum` and `d_ids` are device pointers the engine's streams have finished writing; the pass and
// its folds run on the engine stream and the results are copied back before the call returns.
void surface_launch(bt_engine* e, const bt_summary* d_sum, const int32_t* d_ids, int32_t id_stride,
                    int32_t S, int32_t P, bt_param_agg* agg, bt_topk_rec* best) {
    const SurfacePlan pl = plan_surface(S, P, e->cus, e->surface_chunks);
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_part = 0, o_fold = o_part + up(pl.partial_bytes);
    const size_t o_bpart = o_fold + up(pl.fold_bytes);
    const size_t o_agg = o_bpart + up(pl.best_partial_bytes);
    const size_t o_best = o_agg + up((size_t)P * sizeof(bt_param_agg));
    e->d_surface.ensure(o_best + up((size_t)S * sizeof(bt_topk_rec)) + 256);
    uint8_t* base = e->d_surface.p;
    SurfaceWork w{};
    w.partial = reinterpret_cast<bt_param_agg*>(base + o_part);
    w.fold = reinterpret_cast<bt_param_agg*>(base + o_fold);
    w.best_partial = reinterpret_cast<bt_topk_rec*>(base + o_bpart);
    w.agg = agg ? reinterpret_cast<bt_param_agg*>(base + o_agg) : nullptr;
    w.best = best ? reinterpret_cast<bt_topk_rec*>(base + o_best) : nullptr;
    HIPCHK(launch_surface(d_sum, d_ids, id_stride, S, P, pl, w, e->stream));
    // the results lie next to each other: one copy into pinned memory, whatever was asked for
    const size_t n_agg = (size_t)P * sizeof(bt_param_agg), n_best = (size_t)S * sizeof(bt_topk_rec);
    const size_t lo = agg ? o_agg : o_best, hi = best && S > 0 ? o_best + n_best : o_agg + n_agg;
    if (hi <= lo) return;  // best alone of a matrix without rows
    e->h_surface.ensure(hi - lo);
    HIPCHK(hipMemcpyAsync(e->h_surface.p, base + lo, hi - lo, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (agg) memcpy(agg, e->h_surface.p + (o_agg - lo), n_agg);
    if (best && S > 0) memcpy(best, e->h_surface.p + (o_best - lo), n_best);
}

int32_t surface_impl(bt_engine* e, bt_param_agg* agg, bt_topk_rec* best) {
    auto refuse = [](const std::string& m) { throw HipFail{"bt_surface: " + m}; };
    if (!e) refuse("null engine");
    if (!e->ran) refuse("no results");
    uint64_t rows = 0;
    for (const SymDesc& sd : e->syms) rows += (uint64_t)sd.bars;
    const std::string why = surface_refusal((int64_t)e->syms.size(), e->P, agg || best, false, rows);
    if (!why.empty()) refuse(why);
    activate(e);
    sync_all(e);
    // ids straight from the symbol descriptors: SymDesc is four int32 wide, the id its last
    static_assert(sizeof(SymDesc) == 16 && offsetof(SymDesc, id) == 12, "SymDesc layout");
    surface_launch(e, e->d_sum[e->cur].p, reinterpret_cast<const int32_t*>(e->d_syms.p) + 3, 4,
                   (int32_t)e->syms.size(), e->P, agg, best);
    return 0;
}

int32_t surface_of_impl(bt_engine* e, int32_t S, int32_t P, const bt_summary* sum, const int32_t* ids,
                        bt_param_agg* agg, bt_topk_rec* best) {
    auto refuse = [](const std::string& m) { throw HipFail{"bt_surface_of: " + m}; };
    if (!e) refuse("null engine");
    const std::string why = surface_refusal(S, P, agg || best, true, 0);
    if (!why.empty()) refuse(why);
    if (S > 0 && (!sum || !ids)) refuse("sum and sym_ids are required");
    activate(e);
    sync_all(e);
    const size_t n = (size_t)S * (size_t)P;
    const size_t o_ids = (n * sizeof(bt_summary) + 255) & ~(size_t)255;
    e->d_surface_in.ensure(o_ids + (size_t)S * sizeof(int32_t) + 256);
    uint8_t* base = e->d_surface_in.p;
    if (n) {
        HIPCHK(hipMemcpyAsync(base, sum, n * sizeof(bt_summary), hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(base + o_ids, ids, (size_t)S * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    }
    surface_launch(e, reinterpret_cast<const bt_summary*>(base), reinterpret_cast<const int32_t*>(base + o_ids),
                   1, S, P, agg, best);
    return 0;
}

// ---- bt_walk_forward: every lane's folds and the out-of-sample picks (k_walkfwd.hip)
// The rows go through the device in the chunks of the WalkfwdPlan: per chunk the records are
// zeroed, walked, selected from and copied out; the totals are folded on the host (walkfwd.cpp).
int32_t walk_forward_impl(bt_engine* e, int32_t K, const int32_t* bounds, int32_t train, bt_fold* folds,
                          bt_wf_step* steps, bt_fold* total) {
    auto refuse = [](const std::string& m) { throw HipFail{"bt_walk_forward: " + m}; };
    if (!e) refuse("null engine");
    if (e->syms.empty()) refuse("no dataset loaded");
    if (K >= 1 && !bounds) refuse("bounds are required");
    const int32_t S = (int32_t)e->syms.size(), P = e->P;
    const std::string why = walkfwd_refusal(K, bounds, train, folds != nullptr, steps != nullptr,
                                            total != nullptr, S, P);
    if (!why.empty()) refuse(why);
    const WalkfwdPlan pl = plan_walkfwd(S, P, K, e->max_bars, e->cus, e->walkfwd_budget);
    if (pl.rows_per_chunk < 1)
        refuse("P*K = " + std::to_string(P) + "*" + std::to_string(K) + " records of one row exceed the staging budget of " +
               std::to_string(e->walkfwd_budget > 0 ? (size_t)e->walkfwd_budget : kWalkfwdBudget) + " bytes");
    activate(e);
    sync_all(e);
    const bool select = steps || total;
    const int32_t n_steps = select ? walkfwd_steps(K, train) : 0;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t chunk = (size_t)pl.rows_per_chunk, row_recs = (size_t)K * (size_t)P;
    const size_t o_rec = pl.bounds_bytes, o_steps = o_rec + up(chunk * row_recs * sizeof(bt_fold));
    e->d_walkfwd.ensure(o_steps + up(chunk * (size_t)n_steps * sizeof(bt_wf_step)));
    uint8_t* base = e->d_walkfwd.p;
    HIPCHK(hipMemcpyAsync(base, bounds, ((size_t)K + 1) * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    WfArgs a{};
    a.bounds = reinterpret_cast<const int32_t*>(base);
    a.rec = reinterpret_cast<bt_fold*>(base + o_rec);
    a.steps = reinterpret_cast<bt_wf_step*>(base + o_steps);
    a.P = P, a.K = K;
    a.train = train, a.j0 = std::max(train, 1), a.n_steps = n_steps;
    std::vector<bt_fold> h_rec(folds ? chunk * row_recs : 0);       // device order [row][fold][param]
    std::vector<bt_wf_step> own(!steps && total ? (size_t)S * (size_t)n_steps : 0);
    bt_wf_step* st = steps ? steps : own.data();
    for (size_t r0 = 0; r0 < (size_t)S; r0 += chunk) {
        const size_t m = std::min(chunk, (size_t)S - r0);
        a.syms = e->d_syms.p + r0;
        a.n_rows = (int32_t)m;
        HIPCHK(hipMemsetAsync(a.rec, 0, m * row_recs * sizeof(bt_fold), e->stream));
        HIPCHK(launch_wf_walk(a, e->d_h.p, e->d_l.p, e->d_c.p, e->grid, e->stream));
        if (select) {
            HIPCHK(launch_wf_select(a, e->grid, pl, e->stream));
            HIPCHK(hipMemcpyAsync(st + r0 * (size_t)n_steps, a.steps, m * (size_t)n_steps * sizeof(bt_wf_step),
                                  hipMemcpyDeviceToHost, e->stream));
        }
        if (folds)
            HIPCHK(hipMemcpyAsync(h_rec.data(), a.rec, m * row_recs * sizeof(bt_fold), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        if (folds)   // [row][fold][param] -> the caller's [row][param][fold]
            for (size_t r = 0; r < m; ++r)
                for (size_t k = 0; k < (size_t)K; ++k)
                    for (size_t p = 0; p < (size_t)P; ++p)
                        folds[((r0 + r) * (size_t)P + p) * (size_t)K + k] = h_rec[(r * (size_t)K + k) * (size_t)P + p];
    }
    if (total) walkfwd_totals(S, n_steps, st, e->grid.sqrt_ann, total);
    return 0;
}

void drain_timing(bt_engine* e) {
    for (auto& ev : e->ev_pending) {
        HIPCHK(hipEventSynchronize(ev.second));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, ev.first, ev.second));
        e->kernel_ms += ms;
        e->launches += 1;
        e->ev_pool.push_back(std::move(ev));
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
        HIPCHK(hipEventRecord(e->ev_batch[0], e->stream));
        int32_t* dst[3] = {e->d_c.p, e->d_h.p, e->d_l.p};
        for (int k = 0; k < ncol; ++k)
            HIPCHK(hipMemcpyAsync(dst[k], e->h_stage[k].p, (size_t)rows * 4, hipMemcpyHostToDevice,
                                  e->stream));
        HIPCHK(hipEventRecord(e->ev_batch[1], e->stream));
        run_impl(e);
        HIPCHK(hipEventRecord(e->ev_batch[2], e->stream));
        HIPCHK(hipMemcpyAsync(e->h_sum.p, e->d_sum[e->cur].p, nres * sizeof(bt_summary),
                              hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipEventRecord(e->ev_batch[3], e->stream));
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
    e->tstream.create();
    e->ev_kdone.ensure(hipEventDisableTiming);
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
                          has_hl(e) ? e->d_l.p : nullptr, e->d_c.p, e->stream));
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
                                      hipMemcpyHostToDevice, e->stream));
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

int32_t bt_replay(bt_engine* e, int32_t n, const bt_lane* lanes, int32_t trade_cap, bt_summary* sum,
                  int32_t* n_bars, bt_trade* trades, int64_t* equity, int8_t* pos, int64_t stride) {
    ABI_GUARD(-1, { return replay_impl(e, n, lanes, trade_cap, sum, n_bars, trades, equity, pos, stride); })
}

int32_t bt_surface(bt_engine* e, bt_param_agg* agg, bt_topk_rec* best) {
    ABI_GUARD(-1, { return surface_impl(e, agg, best); })
}

int32_t bt_surface_of(bt_engine* e, int32_t S, int32_t P, const bt_summary* sum, const int32_t* sym_ids,
                      bt_param_agg* agg, bt_topk_rec* best) {
    ABI_GUARD(-1, { return surface_of_impl(e, S, P, sum, sym_ids, agg, best); })
}

int32_t bt_walk_forward(bt_engine* e, int32_t K, const int32_t* bounds, int32_t train, bt_fold* folds,
                        bt_wf_step* steps, bt_fold* total) {
    ABI_GUARD(-1, { return walk_forward_impl(e, K, bounds, train, folds, steps, total); })
}

int32_t bt_set_walkfwd_budget(bt_engine* e, int64_t bytes) {
    ABI_GUARD(-1, {
        if (!e) throw HipFail{"bt_set_walkfwd_budget: null engine"};
        if (bytes < 0) throw HipFail{"bt_set_walkfwd_budget: bytes = " + std::to_string(bytes) + " is negative"};
        e->walkfwd_budget = bytes;
        return 0;
    })
}

int32_t bt_set_surface_chunks(bt_engine* e, int32_t chunks) {
    ABI_GUARD(-1, {
        if (!e) throw HipFail{"bt_set_surface_chunks: null engine"};
        if (chunks < 0) throw HipFail{"bt_set_surface_chunks: chunks = " + std::to_string(chunks) + " is negative"};
        e->surface_chunks = chunks;
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
