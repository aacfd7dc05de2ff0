// engine_state.h — the engine behind the C ABI's bt_engine handle and the helpers its entry points
// share: engine.cpp (lifecycle, datasets, runs, batches) and analysis.cpp (the analysis calls,
// listed at its head). Private to the library and not part of the ABI: it includes HIP.
#pragma once
#include <hip/hip_runtime.h>

#include <utility>
#include <vector>

#include "hip_owned.h"
#include "internal.h"
#include "plan.h"

namespace bt {

constexpr int64_t kNtrRing = 64;  // per-run trade counter slots (EngineState::d_ntr_ring)

struct EngineState {
    bt_config cfg{};
    std::vector<int32_t> ax[4];  // owned copies of the grid axes
    Grid grid{};
    int32_t P = 0;
    // the engine stream (its own, or bt_config.stream borrowed), the run stream (odd runs that may
    // overlap their neighbours, plan.h LaunchPlan::overlap; only beside an owned engine stream) and
    // the top-k chain stream (the chain of run i overlaps the kernel of run i+1). Declared before
    // every buffer and event: members go in reverse order, so the streams outlive what was
    // enqueued on them. Only run_impl enqueues on `stream` or `rstream` by name: every other
    // enqueue asks main_stream() below, which joins the run stream first
    Stream tstream, rstream, stream;
    // What is still enqueued finishes before the members free what it uses. The engine stream is
    // the first HIP object an engine makes: without it there is nothing to wait for.
    ~EngineState() {
        if (!stream) return;
        (void)hipSetDevice(cfg.device);
        (void)hipStreamSynchronize(stream);
        if (rstream) (void)hipStreamSynchronize(rstream);
        if (tstream) (void)hipStreamSynchronize(tstream);
    }
    // The two run streams' ordering against each other (run_impl, main_stream):
    // r_last: the kernel-done event of the last run on the run stream while the engine stream has
    // not been ordered behind it (nullptr: nothing to join); main_dirty: the engine stream holds
    // work, other than overlapping runs, that the run stream has not been ordered behind
    hipEvent_t r_last = nullptr;
    bool main_dirty = false;
    bool overlap_on = true;      // bt_set_run_overlap
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
    Event ev_kdone[2];   // kernel of the last run on the engine stream [0] / the run stream [1] finished
    Event ev_main;       // what the engine stream held when the run stream was last ordered behind it
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
    // timing of the dominant kernel: (start, end) pairs of the runs not yet accounted, spare
    // pairs, and the last accounted run's pair (its end bounds the next run's time from below)
    std::vector<std::pair<Event, Event>> ev_pending, ev_pool;
    std::pair<Event, Event> ev_last;
    double kernel_ms = 0.0;
    int64_t launches = 0;
    // bt_run_batch: pinned host staging of the columns in device row layout (c, h, l), the
    // batch's summaries read back in one copy, phase events and the last batch's profile
    PinnedBuf<int32_t> h_stage[3];
    PinnedBuf<bt_summary> h_sum;
    Event ev_batch[4];
    bt_batch_profile prof{};
    int64_t n_errors = 0;
    // The analysis calls (listed at the head of analysis.cpp) share one device staging arena, grown
    // to the staging_bytes of the current call's plan (plan.h), which lays it out. Sound because
    // every analysis call is synchronous on the engine stream: it drains every stream on entry and
    // the engine stream before it returns, so no two of them are in flight together and nothing
    // reads the arena between calls.
    DevBuf<uint8_t> d_arena;
    int32_t surface_chunks = 0;    // bt_set_surface_chunks (0 = the planner's choice)
    PinnedBuf<uint8_t> h_surface;  // the results of one reduction
    int64_t walkfwd_budget = 0;    // bt_set_walkfwd_budget (0 = kWalkfwdBudget)
    int64_t cscv_work = 0;         // bt_set_cscv_work (0 = kCscvWork)
    int64_t tstats_budget = 0;     // bt_set_tstats_budget (0 = kTstatsBudget)
    int64_t costs_budget = 0;      // bt_set_costs_budget (0 = kCostsBudget)
    int64_t tail_budget = 0;       // bt_set_tail_budget (0 = kTailBudget)
    int32_t tail_row = 0;          // bt_set_tail_row (0 = the planner's choice, 1 = LDS, 2 = arena)
    int32_t last_tail_row = 0;     // bt_last_tail_row: the home the last bt_tail / bt_tail_of used
    int64_t boot_budget = 0;       // bt_set_boot_budget (0 = kBootBudget)
    int32_t boot_row = 0;          // bt_set_boot_row (0 = the planner's choice, 1 = LDS, 2 = arena)
    int64_t ddboot_budget = 0;     // bt_set_ddboot_budget (0 = kDdBudget)
    int32_t ddboot_row = 0;        // bt_set_ddboot_row (0 = the planner's choice, 1 = LDS, 2 = arena)
    int32_t last_ddboot_row = 0;   // bt_last_ddboot_row: the home the last drawdown bootstrap used
    int32_t portfolio_replicas = 0;  // bt_set_portfolio_replicas (0 = the planner's choice)
    PinnedBuf<uint8_t> h_portfolio;  // the rows and the summary of one portfolio
    int32_t gram_split = 0;          // bt_set_gram_split (0 = the planner's choice)
    PinnedBuf<uint8_t> h_gram;       // gram and sums of one covariance
};

}  // namespace bt

struct bt_engine : bt::EngineState {};  // the ABI's opaque handle

namespace bt {

inline void activate(bt_engine* e) { HIPCHK(hipSetDevice(e->cfg.device)); }

inline bool has_hl(const bt_engine* e) { return e->cfg.strategy == BT_BOLL; }

inline void sync_all(bt_engine* e) {
    HIPCHK(hipStreamSynchronize(e->stream));
    if (e->rstream) HIPCHK(hipStreamSynchronize(e->rstream));
    e->r_last = nullptr;
    if (e->tstream) HIPCHK(hipStreamSynchronize(e->tstream));
}

// The engine stream for anything but an overlapping run's kernel: loads, read-backs, analysis
// calls, the counter ring's zeroing, runs that may not overlap. What it enqueues is ordered behind
// the run stream's last kernel (no wait packet when that kernel has already finished), and the
// next run on the run stream is ordered behind it (run_impl).
inline hipStream_t main_stream(bt_engine* e) {
    if (e->r_last) {
        if (hipEventQuery(e->r_last) != hipSuccess) HIPCHK(hipStreamWaitEvent(e->stream, e->r_last, 0));
        e->r_last = nullptr;
    }
    e->main_dirty = true;
    return e->stream;
}

// The one cast from a staging offset (plan.h Carve) to a typed device pointer.
template <class T>
T* at(uint8_t* base, size_t off) { return reinterpret_cast<T*>(base + off); }

}  // namespace bt
