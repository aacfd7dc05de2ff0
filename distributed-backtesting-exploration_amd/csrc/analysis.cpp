// analysis.cpp — the analysis calls of the C ABI: bt_replay, bt_surface, bt_surface_of, bt_topk_of,
// bt_walk_forward, bt_cscv, bt_cscv_of, bt_trade_stats, bt_costs, bt_tail, bt_tail_of, bt_bootstrap,
// bt_bootstrap_of, bt_drawdown_boot, bt_drawdown_boot_of, bt_portfolio, bt_covariance and bt_gram_of,
// with their settings (bt_set_*). This
// is the list the other files point to. Each call checks its arguments with the pure rules of its
// header (replay.h, surface.h, topk_rules.h, walkfwd.h, cscv.h, tstats.h, costs.h, tail.h,
// bootstrap.h, ddboot.h, portfolio.h, covariance.h), asks plan.h for its chunks and its staging layout,
// realises that layout in the engine's one arena
// (engine_state.h), launches, and copies the results back before it returns. Nothing is computed on
// the CPU but the walk-forward totals (walkfwd.cpp).
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "bootstrap.h"
#include "costs.h"
#include "covariance.h"
#include "cscv.h"
#include "ddboot.h"
#include "engine_state.h"
#include "portfolio.h"
#include "replay.h"
#include "surface.h"
#include "tail.h"
#include "topk_rules.h"
#include "tstats.h"
#include "walkfwd.h"

using namespace bt;

namespace {

// In this file a refusal throws (ABI_GUARD turns it into bt_last_error() and -1): a bare
// `refuse(fn, why);` ends the call. It hides bt::refuse of host_common.h, which returns -1 and is
// what the HIP-free files `return`.
[[noreturn]] void refuse(const char* fn, const std::string& why) { throw HipFail{std::string(fn) + ": " + why}; }

// Every analysis call starts here, after its refusals: every stream drained, then the arena grown
// to the call's plan. With the wait on the engine stream before the call returns this is the
// invariant the shared arena rests on (engine_state.h).
uint8_t* enter(bt_engine* e, size_t staging_bytes) {
    activate(e);
    sync_all(e);
    e->d_arena.ensure(staging_bytes);
    return e->d_arena.p;
}

// fn(first, count) for every chunk of `per` out of n items, in order; the last one may be shorter.
template <class F>
void for_chunks(size_t n, size_t per, F fn) {
    for (size_t i0 = 0; i0 < n; i0 += per) fn(i0, std::min(per, n - i0));
}

// List mode of bt_trade_stats, bt_bootstrap and bt_covariance: the n requests against the dataset,
// or the refusal. W: the longest requested symbol.
std::vector<LaneRef> resolve(bt_engine* e, const char* fn, int32_t n, const bt_lane* lanes, int32_t& W) {
    std::vector<LaneRef> req;
    const std::string why = lanes_resolve(e->syms.data(), e->syms.size(), e->P, n, lanes, req, W);
    if (!why.empty()) refuse(fn, why);
    return req;
}

// A setting of the analysis calls (bt_set_*): v in [0, hi], or v >= 0 with hi < 0, into its field.
template <class T>
int32_t set_knob(bt_engine* e, const char* fn, const char* arg, int64_t v, int64_t hi, T EngineState::*field) {
    if (!e) refuse(fn, "null engine");
    if (hi < 0 && v < 0) refuse(fn, std::string(arg) + " = " + std::to_string(v) + " is negative");
    if (hi >= 0 && (v < 0 || v > hi))
        refuse(fn, std::string(arg) + " = " + std::to_string(v) + " outside [0, " + std::to_string(hi) + "]");
    e->*field = (T)v;
    return 0;
}

// ---- bt_replay: chosen lanes again, with their trades and curves (k_replay.hip)
int32_t replay_impl(bt_engine* e, int32_t n, const bt_lane* lanes, int32_t trade_cap, bt_summary* sum,
                    int32_t* n_bars, bt_trade* trades, int64_t* equity, int8_t* pos, int64_t stride) {
    const char* fn = "bt_replay";
    if (!e) refuse(fn, "null engine");
    std::string why = replay_refusal(!e->syms.empty(), n, trade_cap, trades != nullptr, lanes != nullptr, sum != nullptr);
    if (!why.empty()) refuse(fn, why);
    if (n == 0) return 0;
    std::vector<LaneRef> req;
    int32_t W = 0;  // the longest requested symbol
    why = replay_resolve(e->syms.data(), e->syms.size(), e->P, n, lanes, equity || pos, stride, req, W);
    if (!why.empty()) refuse(fn, why);
    const ReplayPlan pl = plan_replay(n, W, trade_cap, stride, equity != nullptr, pos != nullptr);
    uint8_t* base = enter(e, pl.staging_bytes);
    const size_t dcap = (size_t)pl.dcap, pitch = (size_t)pl.pitch;
    LaneRef* d_lanes = at<LaneRef>(base, pl.o_lane);
    ReplayOut out{};
    out.sum = at<bt_summary>(base, pl.o_sum);
    out.trades = dcap ? at<bt_trade>(base, pl.o_trades) : nullptr;
    out.trade_cap = (int32_t)dcap;
    out.equity = equity ? at<int64_t>(base, pl.o_equity) : nullptr;
    out.pos = pos ? at<int8_t>(base, pl.o_pos) : nullptr;
    out.pitch = pl.pitch;
    // rows of a host array -> rows of a device one: one copy when the pitches agree, else a 2-D
    // copy and the host tails zeroed here
    auto fetch = [&](void* dst, size_t dst_pitch, const void* src, size_t src_pitch, size_t m) {
        if (dst_pitch == src_pitch) {
            HIPCHK(hipMemcpyAsync(dst, src, m * src_pitch, hipMemcpyDeviceToHost, main_stream(e)));
            return;
        }
        HIPCHK(hipMemcpy2DAsync(dst, dst_pitch, src, src_pitch, src_pitch, m, hipMemcpyDeviceToHost, main_stream(e)));
        for (size_t i = 0; i < m; ++i)
            memset(static_cast<uint8_t*>(dst) + i * dst_pitch + src_pitch, 0, dst_pitch - src_pitch);
    };
    for_chunks((size_t)n, (size_t)pl.lanes_per_chunk, [&](size_t i0, size_t m) {
        HIPCHK(hipMemcpyAsync(d_lanes, req.data() + i0, m * sizeof(LaneRef), hipMemcpyHostToDevice, main_stream(e)));
        if (dcap) HIPCHK(hipMemsetAsync(out.trades, 0, m * dcap * sizeof(bt_trade), main_stream(e)));
        if (equity) HIPCHK(hipMemsetAsync(out.equity, 0, m * pitch * 8, main_stream(e)));
        if (pos) HIPCHK(hipMemsetAsync(out.pos, 0, m * pitch, main_stream(e)));
        HIPCHK(launch_replay(d_lanes, (int32_t)m, e->d_h.p, e->d_l.p, e->d_c.p, e->grid, out, main_stream(e)));
        HIPCHK(hipMemcpyAsync(sum + i0, out.sum, m * sizeof(bt_summary), hipMemcpyDeviceToHost, main_stream(e)));
        if (dcap)
            fetch(trades + i0 * (size_t)trade_cap, (size_t)trade_cap * sizeof(bt_trade), out.trades,
                  dcap * sizeof(bt_trade), m);
        if (equity) fetch(equity + i0 * (size_t)stride, (size_t)stride * 8, out.equity, pitch * 8, m);
        if (pos) fetch(pos + i0 * (size_t)stride, (size_t)stride, out.pos, pitch, m);
        HIPCHK(hipStreamSynchronize(main_stream(e)));
    });
    if (n_bars)
        for (int32_t i = 0; i < n; ++i) n_bars[i] = req[i].bars;
    return n;
}

// ---- bt_surface / bt_surface_of: the run's summaries reduced on the device (k_surface.hip)
// `d_sum` and `d_ids` are device pointers the engine's streams have finished writing; the pass and
// its folds run on the engine stream and the results are copied back before the call returns.
void surface_launch(bt_engine* e, const SurfacePlan& pl, uint8_t* base, const bt_summary* d_sum,
                    const int32_t* d_ids, int32_t id_stride, int32_t S, int32_t P, bt_param_agg* agg,
                    bt_topk_rec* best) {
    SurfaceWork w{};
    w.partial = at<bt_param_agg>(base, pl.o_partial);
    w.fold = at<bt_param_agg>(base, pl.o_fold);
    w.best_partial = at<bt_topk_rec>(base, pl.o_best_partial);
    w.agg = agg ? at<bt_param_agg>(base, pl.o_agg) : nullptr;
    w.best = best ? at<bt_topk_rec>(base, pl.o_best) : nullptr;
    HIPCHK(launch_surface(d_sum, d_ids, id_stride, S, P, pl, w, main_stream(e)));
    // the results lie next to each other: one copy into pinned memory, whatever was asked for
    const size_t n_agg = (size_t)P * sizeof(bt_param_agg), n_best = (size_t)S * sizeof(bt_topk_rec);
    const size_t lo = agg ? pl.o_agg : pl.o_best, hi = best && S > 0 ? pl.o_best + n_best : pl.o_agg + n_agg;
    if (hi <= lo) return;  // best alone of a matrix without rows
    e->h_surface.ensure(hi - lo);
    HIPCHK(hipMemcpyAsync(e->h_surface.p, base + lo, hi - lo, hipMemcpyDeviceToHost, main_stream(e)));
    HIPCHK(hipStreamSynchronize(main_stream(e)));
    if (agg) memcpy(agg, e->h_surface.p + (pl.o_agg - lo), n_agg);
    if (best && S > 0) memcpy(best, e->h_surface.p + (pl.o_best - lo), n_best);
}

int32_t surface_impl(bt_engine* e, bt_param_agg* agg, bt_topk_rec* best) {
    const char* fn = "bt_surface";
    if (!e) refuse(fn, "null engine");
    if (!e->ran) refuse(fn, "no results");
    uint64_t rows = 0;
    for (const SymDesc& sd : e->syms) rows += (uint64_t)sd.bars;
    const int32_t S = (int32_t)e->syms.size();
    const std::string why = surface_refusal(S, e->P, agg || best, false, rows);
    if (!why.empty()) refuse(fn, why);
    const SurfacePlan pl = plan_surface(S, e->P, e->cus, e->surface_chunks);
    uint8_t* base = enter(e, pl.staging_bytes);
    // ids straight from the symbol descriptors: SymDesc is four int32 wide, the id its last
    static_assert(sizeof(SymDesc) == 16 && offsetof(SymDesc, id) == 12, "SymDesc layout");
    surface_launch(e, pl, base, e->d_sum[e->cur].p, reinterpret_cast<const int32_t*>(e->d_syms.p) + 3, 4, S,
                   e->P, agg, best);
    return 0;
}

int32_t surface_of_impl(bt_engine* e, int32_t S, int32_t P, const bt_summary* sum, const int32_t* ids,
                        bt_param_agg* agg, bt_topk_rec* best) {
    const char* fn = "bt_surface_of";
    if (!e) refuse(fn, "null engine");
    const std::string why = surface_refusal(S, P, agg || best, true, 0);
    if (!why.empty()) refuse(fn, why);
    if (S > 0 && (!sum || !ids)) refuse(fn, "sum and sym_ids are required");
    const SurfacePlan pl = plan_surface(S, P, e->cus, e->surface_chunks, true);
    uint8_t* base = enter(e, pl.staging_bytes);
    bt_summary* d_sum = at<bt_summary>(base, pl.o_sum);
    int32_t* d_ids = at<int32_t>(base, pl.o_ids);
    if (S > 0) {
        HIPCHK(hipMemcpyAsync(d_sum, sum, (size_t)S * (size_t)P * sizeof(bt_summary), hipMemcpyHostToDevice, main_stream(e)));
        HIPCHK(hipMemcpyAsync(d_ids, ids, (size_t)S * sizeof(int32_t), hipMemcpyHostToDevice, main_stream(e)));
    }
    surface_launch(e, pl, base, d_sum, d_ids, 1, S, P, agg, best);
    return 0;
}

// ---- bt_topk_of: the run's top-k chain (k_topk.hip) on a caller's records
// The keys are what a strategy kernel would have left beside these summaries (order_key of the
// Sharpe), the descriptors carry the ids alone (the chain reads nothing else of them), and the
// TopkWork is the call's own, in the arena: the engine's d_top, its selection state and its key
// buffers stay as the last run left them.
int32_t topk_of_impl(bt_engine* e, int32_t S, int32_t P, const bt_summary* sum, const int32_t* ids, int32_t k,
                     int32_t lds_free_hist, bt_topk_rec* out) {
    static_assert(kTopkOfMaxK == kTopkMax, "topk_rules.h restates kTopkMax");
    const char* fn = "bt_topk_of";
    if (!e) refuse(fn, "null engine");
    const std::string why = topk_of_refusal(S, P, k, sum != nullptr, ids, out != nullptr);
    if (!why.empty()) refuse(fn, why);
    const size_t n = (size_t)S * (size_t)P;
    std::vector<uint64_t> key(n);
    for (size_t i = 0; i < n; ++i) key[i] = order_key(sum[i].sharpe);
    std::vector<SymDesc> syms((size_t)S);
    for (int32_t s = 0; s < S; ++s) syms[s] = SymDesc{0, 0, ids[s]};
    const TopkOfPlan pl = plan_topk_of(S, P);
    uint8_t* base = enter(e, pl.staging_bytes);
    uint64_t* d_key = at<uint64_t>(base, pl.o_key);
    bt_summary* d_sum = at<bt_summary>(base, pl.o_sum);
    SymDesc* d_syms = at<SymDesc>(base, pl.o_syms);
    bt_topk_rec* d_out = at<bt_topk_rec>(base, pl.o_out);  // [0]: the count, then the records
    const TopkWork w{at<unsigned int>(base, pl.o_hist),      at<unsigned long long>(base, pl.o_state),
                     at<unsigned int>(base, pl.o_counts),    at<unsigned long long>(base, pl.o_above),
                     at<unsigned long long>(base, pl.o_cand), kTopkCap, d_out + 1, reinterpret_cast<int32_t*>(d_out)};
    HIPCHK(hipMemcpyAsync(d_key, key.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice, main_stream(e)));
    HIPCHK(hipMemcpyAsync(d_sum, sum, n * sizeof(bt_summary), hipMemcpyHostToDevice, main_stream(e)));
    HIPCHK(hipMemcpyAsync(d_syms, syms.data(), (size_t)S * sizeof(SymDesc), hipMemcpyHostToDevice, main_stream(e)));
    HIPCHK(hipMemsetAsync(d_out, 0, ((size_t)kTopkMax + 1) * sizeof(bt_topk_rec), main_stream(e)));
    HIPCHK(launch_topk_init(w, main_stream(e)));
    HIPCHK(launch_topk(d_key, d_sum, d_syms, (int64_t)n, P, k, w, main_stream(e), lds_free_hist != 0));
    std::vector<bt_topk_rec> got((size_t)k + 1);
    HIPCHK(hipMemcpyAsync(got.data(), d_out, got.size() * sizeof(bt_topk_rec), hipMemcpyDeviceToHost, main_stream(e)));
    HIPCHK(hipStreamSynchronize(main_stream(e)));
    int32_t count;
    memcpy(&count, &got[0], sizeof count);
    if (count < 0 || count > k) refuse(fn, "the device wrote a count of " + std::to_string(count));
    memcpy(out, got.data() + 1, (size_t)count * sizeof(bt_topk_rec));
    return count;
}

// ---- bt_walk_forward: every lane's folds and the out-of-sample picks (k_walkfwd.hip)
// The rows go through the device in the chunks of the WalkfwdPlan: per chunk the records are
// zeroed, walked, selected from and copied out; the totals are folded on the host (walkfwd.cpp).
int32_t walk_forward_impl(bt_engine* e, int32_t K, const int32_t* bounds, int32_t train, bt_fold* folds,
                          bt_wf_step* steps, bt_fold* total) {
    const char* fn = "bt_walk_forward";
    if (!e) refuse(fn, "null engine");
    if (e->syms.empty()) refuse(fn, "no dataset loaded");
    if (K >= 1 && !bounds) refuse(fn, "bounds are required");
    const int32_t S = (int32_t)e->syms.size(), P = e->P;
    const std::string why = walkfwd_refusal(K, bounds, train, folds != nullptr, steps != nullptr,
                                            total != nullptr, S, P);
    if (!why.empty()) refuse(fn, why);
    const WalkfwdPlan pl = plan_walkfwd(S, P, K, e->max_bars, e->cus, e->walkfwd_budget);
    if (pl.rows_per_chunk < 1)
        refuse(fn, "P*K = " + std::to_string(P) + "*" + std::to_string(K) + " records of one row exceed the staging budget of " +
                       std::to_string(e->walkfwd_budget > 0 ? (size_t)e->walkfwd_budget : kWalkfwdBudget) + " bytes");
    uint8_t* base = enter(e, pl.staging_bytes);
    const bool select = steps || total;
    const int32_t n_steps = select ? walkfwd_steps(K, train) : 0;
    const size_t row_recs = (size_t)K * (size_t)P;
    HIPCHK(hipMemcpyAsync(base, bounds, ((size_t)K + 1) * sizeof(int32_t), hipMemcpyHostToDevice, main_stream(e)));
    WfArgs a{};
    a.bounds = at<const int32_t>(base, 0);
    a.rec = at<bt_fold>(base, pl.o_rec);
    a.steps = at<bt_wf_step>(base, pl.o_steps);
    a.P = P, a.K = K;
    a.train = train, a.j0 = std::max(train, 1), a.n_steps = n_steps;
    std::vector<bt_fold> h_rec(folds ? (size_t)pl.rows_per_chunk * row_recs : 0);  // device order [row][fold][param]
    std::vector<bt_wf_step> own(!steps && total ? (size_t)S * (size_t)n_steps : 0);
    bt_wf_step* st = steps ? steps : own.data();
    for_chunks((size_t)S, (size_t)pl.rows_per_chunk, [&](size_t r0, size_t m) {
        a.syms = e->d_syms.p + r0;
        a.n_rows = (int32_t)m;
        HIPCHK(hipMemsetAsync(a.rec, 0, m * row_recs * sizeof(bt_fold), main_stream(e)));
        HIPCHK(launch_wf_walk(a, e->d_h.p, e->d_l.p, e->d_c.p, e->grid, main_stream(e)));
        if (select) {
            HIPCHK(launch_wf_select(a, e->grid, pl, main_stream(e)));
            HIPCHK(hipMemcpyAsync(st + r0 * (size_t)n_steps, a.steps, m * (size_t)n_steps * sizeof(bt_wf_step),
                                  hipMemcpyDeviceToHost, main_stream(e)));
        }
        if (folds)
            HIPCHK(hipMemcpyAsync(h_rec.data(), a.rec, m * row_recs * sizeof(bt_fold), hipMemcpyDeviceToHost, main_stream(e)));
        HIPCHK(hipStreamSynchronize(main_stream(e)));
        if (folds)   // [row][fold][param] -> the caller's [row][param][fold]
            for (size_t r = 0; r < m; ++r)
                for (size_t k = 0; k < (size_t)K; ++k)
                    for (size_t p = 0; p < (size_t)P; ++p)
                        folds[((r0 + r) * (size_t)P + p) * (size_t)K + k] = h_rec[(r * (size_t)K + k) * (size_t)P + p];
    });
    if (total) walkfwd_totals(S, n_steps, st, e->grid.sqrt_ann, total);
    return 0;
}

// ---- bt_cscv / bt_cscv_of: the probability of backtest overfitting (k_cscv.hip)
// The groups go through the device in the chunks of the CscvPlan: per chunk the fold records are
// walked (bt_cscv: `folds` is NULL, the groups are the dataset's rows) or uploaded (bt_cscv_of) and
// packed, the group records and histograms zeroed, the combination kernel launched as often as the
// plan's launch cap asks, and the results copied out. The host adds only what no kernel computes:
// every group's id and lane count.
int32_t cscv_run(bt_engine* e, const char* fn, int32_t G, int32_t P, int32_t K, const int32_t* bounds,
                 const bt_fold* folds, const int32_t* sym_ids, bt_cscv_group* groups, uint32_t* hist,
                 bt_cscv_pick* picks) {
    if (G == 0) return 0;
    const CscvPlan pl = plan_cscv(G, P, K, picks != nullptr, e->walkfwd_budget, e->cscv_work);
    if (pl.rows_per_chunk < 1)
        refuse(fn, "one row of P = " + std::to_string(P) + " lanes and K = " + std::to_string(K) + " folds needs " +
                       std::to_string(pl.row_bytes) + " bytes, above the staging budget of " +
                       std::to_string(e->walkfwd_budget > 0 ? (size_t)e->walkfwd_budget : kWalkfwdBudget) + " bytes");
    uint8_t* base = enter(e, pl.staging_bytes);
    const size_t row_recs = (size_t)K * (size_t)P, H = 2 * (size_t)P - 1, C = (size_t)pl.C;
    if (bounds)
        HIPCHK(hipMemcpyAsync(base, bounds, ((size_t)K + 1) * sizeof(int32_t), hipMemcpyHostToDevice, main_stream(e)));
    HIPCHK(hipMemcpyAsync(base + pl.o_masks, pl.masks.data(), pl.masks.size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                          main_stream(e)));
    WfArgs w{};
    w.bounds = at<const int32_t>(base, 0);
    w.rec = at<bt_fold>(base, pl.o_rec);
    w.P = P, w.K = K;
    CscvArgs a{};
    a.rec = w.rec;
    a.stride_p = folds ? K : 1, a.stride_k = folds ? 1 : P;   // staged [P][K]; the walk's [K][P]
    a.sums = at<CscvSum>(base, pl.o_sums);
    a.nret = at<int32_t>(base, pl.o_nret);
    a.masks = at<const uint32_t>(base, pl.o_masks);
    a.groups = at<bt_cscv_group>(base, pl.o_groups);
    a.hist = hist ? at<uint32_t>(base, pl.o_hist) : nullptr;
    a.picks = picks ? at<bt_cscv_pick>(base, pl.o_picks) : nullptr;
    a.P = P, a.K = K, a.C = pl.C, a.pairs = pl.pairs;
    for_chunks((size_t)G, (size_t)pl.rows_per_chunk, [&](size_t r0, size_t m) {
        a.n_rows = (int32_t)m;
        if (folds) {
            HIPCHK(hipMemcpyAsync(w.rec, folds + r0 * row_recs, m * row_recs * sizeof(bt_fold), hipMemcpyHostToDevice,
                                  main_stream(e)));
        } else {
            w.syms = e->d_syms.p + r0;
            w.n_rows = (int32_t)m;
            HIPCHK(hipMemsetAsync(w.rec, 0, m * row_recs * sizeof(bt_fold), main_stream(e)));
            HIPCHK(launch_wf_walk(w, e->d_h.p, e->d_l.p, e->d_c.p, e->grid, main_stream(e)));
        }
        HIPCHK(launch_cscv_pack(a, pl, main_stream(e)));
        HIPCHK(hipMemsetAsync(a.groups, 0, m * sizeof(bt_cscv_group), main_stream(e)));
        if (hist) HIPCHK(hipMemsetAsync(a.hist, 0, m * H * sizeof(uint32_t), main_stream(e)));
        for_chunks(m, (size_t)pl.rows_per_launch, [&](size_t l0, size_t rows) {
            for_chunks((size_t)pl.pairs, (size_t)pl.pairs_per_launch, [&](size_t q0, size_t nq) {
                HIPCHK(launch_cscv(a, pl, (int32_t)l0, (int32_t)rows, (int64_t)q0, (int64_t)(q0 + nq), e->grid.sqrt_ann,
                                   main_stream(e)));
            });
        });
        bt_cscv_group* g = groups ? groups + r0 : nullptr;
        if (g) HIPCHK(hipMemcpyAsync(g, a.groups, m * sizeof(bt_cscv_group), hipMemcpyDeviceToHost, main_stream(e)));
        if (hist) HIPCHK(hipMemcpyAsync(hist + r0 * H, a.hist, m * H * sizeof(uint32_t), hipMemcpyDeviceToHost, main_stream(e)));
        if (picks)
            HIPCHK(hipMemcpyAsync(picks + r0 * C, a.picks, m * C * sizeof(bt_cscv_pick), hipMemcpyDeviceToHost, main_stream(e)));
        HIPCHK(hipStreamSynchronize(main_stream(e)));
        if (g)
            for (size_t r = 0; r < m; ++r) {
                g[r].sym = folds ? (sym_ids ? sym_ids[r0 + r] : (int32_t)(r0 + r)) : e->syms[r0 + r].id;
                g[r].n_lanes = P;
            }
    });
    return 0;
}

int32_t cscv_impl(bt_engine* e, int32_t K, const int32_t* bounds, bt_cscv_group* groups, uint32_t* hist,
                  bt_cscv_pick* picks) {
    const char* fn = "bt_cscv";
    if (!e) refuse(fn, "null engine");
    if (e->syms.empty()) refuse(fn, "no dataset loaded");
    if (K >= 1 && !bounds) refuse(fn, "bounds are required");
    const int32_t S = (int32_t)e->syms.size();
    const std::string why = cscv_refusal(K, bounds, groups != nullptr, hist != nullptr, picks != nullptr, S);
    if (!why.empty()) refuse(fn, why);
    return cscv_run(e, fn, S, e->P, K, bounds, nullptr, nullptr, groups, hist, picks);
}

int32_t cscv_of_impl(bt_engine* e, int32_t G, int32_t P, int32_t K, const bt_fold* folds, const int32_t* sym_ids,
                     bt_cscv_group* groups, uint32_t* hist, bt_cscv_pick* picks) {
    const char* fn = "bt_cscv_of";
    if (!e) refuse(fn, "null engine");
    std::string why = cscv_refusal(K, nullptr, groups != nullptr, hist != nullptr, picks != nullptr, std::max(G, 0));
    if (why.empty()) why = cscv_folds_refusal(G, P, K, folds);
    if (!why.empty()) refuse(fn, why);
    return cscv_run(e, fn, G, P, K, nullptr, folds, sym_ids, groups, hist, picks);
}

// ---- bt_trade_stats: every lane's, or chosen lanes', trade statistics (k_tstats.hip)
// The rows (all-lanes mode) or the requests (list mode) go through the device in the chunks of the
// TstatsPlan: per chunk the walk leaves its records, which are copied out when `out` is given and
// reduced into agg[P] on the device when `agg` is; agg comes back once, after the last chunk.
int32_t trade_stats_impl(bt_engine* e, int32_t n, const bt_lane* lanes, bt_tstats* out, bt_tstats_agg* agg) {
    const char* fn = "bt_trade_stats";
    if (!e) refuse(fn, "null engine");
    std::string why = tstats_refusal(!e->syms.empty(), n, lanes != nullptr, out != nullptr, agg != nullptr);
    if (!why.empty()) refuse(fn, why);
    const bool list = lanes != nullptr;
    if (list && n == 0) return 0;
    const int32_t S = (int32_t)e->syms.size(), P = e->P;
    int32_t W = 0;
    const std::vector<LaneRef> req = list ? resolve(e, fn, n, lanes, W) : std::vector<LaneRef>{};
    const TstatsPlan pl = plan_tstats(list ? n : S, P, list, e->cus, e->tstats_budget);
    if (pl.per_chunk < 1)   // list mode: the record of one lane
        refuse(fn, tstats_budget_refusal(list ? 1 : P, e->tstats_budget > 0 ? e->tstats_budget : (int64_t)kTstatsBudget));
    uint8_t* base = enter(e, pl.staging_bytes);
    TsArgs a{};
    a.rec = at<bt_tstats>(base, pl.o_rec);
    a.agg = agg ? at<bt_tstats_agg>(base, pl.o_agg) : nullptr;
    a.P = P;
    LaneRef* d_lanes = list ? at<LaneRef>(base, pl.o_lanes) : nullptr;
    if (agg) HIPCHK(hipMemsetAsync(a.agg, 0, (size_t)P * sizeof(bt_tstats_agg), main_stream(e)));
    const size_t unit_recs = list ? 1 : (size_t)P;
    for_chunks(list ? (size_t)n : (size_t)S, (size_t)pl.per_chunk, [&](size_t i0, size_t m) {
        if (list) {
            HIPCHK(hipMemcpyAsync(d_lanes, req.data() + i0, m * sizeof(LaneRef), hipMemcpyHostToDevice, main_stream(e)));
            a.lanes = d_lanes;
            a.n = (int32_t)m;
        } else {
            a.syms = e->d_syms.p + i0;
            a.n_rows = (int32_t)m;
        }
        HIPCHK(launch_tstats_walk(a, e->d_h.p, e->d_l.p, e->d_c.p, e->grid, main_stream(e)));
        if (agg) HIPCHK(launch_tstats_agg(a, pl, main_stream(e)));
        if (out)
            HIPCHK(hipMemcpyAsync(out + i0 * unit_recs, a.rec, m * unit_recs * sizeof(bt_tstats), hipMemcpyDeviceToHost,
                                  main_stream(e)));
        HIPCHK(hipStreamSynchronize(main_stream(e)));
    });
    if (agg) {
        HIPCHK(hipMemcpyAsync(agg, a.agg, (size_t)P * sizeof(bt_tstats_agg), hipMemcpyDeviceToHost, main_stream(e)));
        HIPCHK(hipStreamSynchronize(main_stream(e)));
    }
    return 0;
}

// ---- bt_costs: every lane, or chosen lanes, under a ladder of fee levels (k_costs.hip)
// The chunks of bt_trade_stats with C records per lane (CostsPlan); the level table goes to the
// walk by value.
int32_t costs_impl(bt_engine* e, int32_t C, const int32_t* levels, int32_t n, const bt_lane* lanes, bt_cost_rec* out,
                   bt_cost_agg* agg) {
    const char* fn = "bt_costs";
    if (!e) refuse(fn, "null engine");
    std::string why = costs_refusal(!e->syms.empty(), C, levels, n, lanes != nullptr, out != nullptr, agg != nullptr);
    if (!why.empty()) refuse(fn, why);
    const bool list = lanes != nullptr;
    if (list && n == 0) return 0;
    const int32_t S = (int32_t)e->syms.size(), P = e->P;
    int32_t W = 0;
    const std::vector<LaneRef> req = list ? resolve(e, fn, n, lanes, W) : std::vector<LaneRef>{};
    const CostsPlan pl = plan_costs(list ? n : S, P, C, list, e->cus, e->costs_budget);
    if (pl.per_chunk < 1)   // list mode: the records of one lane
        refuse(fn, costs_budget_refusal(list ? 1 : P, C, e->costs_budget > 0 ? e->costs_budget : (int64_t)kCostsBudget));
    uint8_t* base = enter(e, pl.staging_bytes);
    CostLevels lv{};
    for (int32_t j = 0; j < C; ++j) lv.fixed[j] = levels[2 * j], lv.bps[j] = levels[2 * j + 1];
    CostArgs a{};
    a.rec = at<bt_cost_rec>(base, pl.o_rec);
    a.agg = agg ? at<bt_cost_agg>(base, pl.o_agg) : nullptr;
    a.P = P;
    a.C = C;
    LaneRef* d_lanes = list ? at<LaneRef>(base, pl.o_lanes) : nullptr;
    const size_t PC = (size_t)P * (size_t)C;
    if (agg) HIPCHK(hipMemsetAsync(a.agg, 0, PC * sizeof(bt_cost_agg), main_stream(e)));
    const size_t unit_recs = list ? (size_t)C : PC;
    for_chunks(list ? (size_t)n : (size_t)S, (size_t)pl.per_chunk, [&](size_t i0, size_t m) {
        if (list) {
            HIPCHK(hipMemcpyAsync(d_lanes, req.data() + i0, m * sizeof(LaneRef), hipMemcpyHostToDevice, main_stream(e)));
            a.lanes = d_lanes;
            a.n = (int32_t)m;
        } else {
            a.syms = e->d_syms.p + i0;
            a.n_rows = (int32_t)m;
        }
        HIPCHK(launch_cost_walk(a, lv, e->d_h.p, e->d_l.p, e->d_c.p, e->grid, main_stream(e)));
        if (agg) HIPCHK(launch_cost_agg(a, pl, main_stream(e)));
        if (out)
            HIPCHK(hipMemcpyAsync(out + i0 * unit_recs, a.rec, m * unit_recs * sizeof(bt_cost_rec), hipMemcpyDeviceToHost,
                                  main_stream(e)));
        HIPCHK(hipStreamSynchronize(main_stream(e)));
    });
    if (agg) {
        HIPCHK(hipMemcpyAsync(agg, a.agg, PC * sizeof(bt_cost_agg), hipMemcpyDeviceToHost, main_stream(e)));
        HIPCHK(hipStreamSynchronize(main_stream(e)));
    }
    return 0;
}

// ---- bt_tail / bt_tail_of: per-lane moments and lower-tail order statistics (k_tail.hip)
// `req`: the resolved lanes of a list call; `d`: the increments of a staged call (rows of T); neither:
// every lane of the dataset, `units` rows of P. `longest_n`: the most bars a lane can count. The
// levels go up once; every chunk uploads its requests or its rows, runs one workgroup per lane and
// brings its records back.
int32_t tail_run(bt_engine* e, const char* fn, int32_t units, const std::vector<LaneRef>* req, const int32_t* d,
                 int32_t longest_n, int32_t from, int32_t to, int32_t mode, int32_t Q, const int32_t* alpha_ppm,
                 bt_tail_rec* recs, bt_tail_q* q) {
    const bool list = req != nullptr, staged = d != nullptr;
    const size_t P = list || staged ? 1 : (size_t)e->P;
    const TailPlan pl = plan_tail(units, (int32_t)P, Q, list, staged, longest_n, e->cus, e->tail_row, e->tail_budget);
    if (pl.row_refused) refuse(fn, tail_row_refusal(longest_n, (size_t)longest_n * 4, (size_t)pl.lds_row_cap * 4));
    if (pl.per_chunk < 1)
        refuse(fn, tail_budget_refusal(!list && !staged, pl.need_bytes, e->tail_budget > 0 ? (size_t)e->tail_budget : kTailBudget));
    uint8_t* base = enter(e, pl.staging_bytes);
    hipStream_t st = main_stream(e);
    e->last_tail_row = pl.row_mode;
    TailArgs a{};
    a.levels = at<const int32_t>(base, pl.o_levels);
    a.rec = recs ? at<bt_tail_rec>(base, pl.o_rec) : nullptr;
    a.q = q ? at<bt_tail_q>(base, pl.o_q) : nullptr;
    a.rows = pl.pitch > 0 ? at<int32_t>(base, pl.o_rows) : nullptr;
    a.pitch = pl.pitch;
    a.P = (int32_t)P, a.Q = Q;
    a.from = from, a.to = to, a.held = mode == BT_TAIL_HELD ? 1 : 0;
    a.T = staged ? longest_n : 0;
    a.cap = longest_n;
    LaneRef* d_lanes = list ? at<LaneRef>(base, pl.o_lanes) : nullptr;
    HIPCHK(hipMemcpyAsync(base + pl.o_levels, alpha_ppm, (size_t)Q * 4, hipMemcpyHostToDevice, st));
    for_chunks((size_t)units, (size_t)pl.per_chunk, [&](size_t i0, size_t m) {
        const size_t lanes = m * P;
        if (list) {
            HIPCHK(hipMemcpyAsync(d_lanes, req->data() + i0, m * sizeof(LaneRef), hipMemcpyHostToDevice, st));
            a.lanes = d_lanes;
        } else if (staged) {
            const size_t T = (size_t)longest_n;
            HIPCHK(hipMemcpy2DAsync(a.rows, (size_t)pl.pitch * 4, d + i0 * T, T * 4, T * 4, m, hipMemcpyHostToDevice, st));
        } else {
            a.syms = e->d_syms.p + i0;
        }
        if (staged) HIPCHK(launch_tail_of(a, (int32_t)lanes, pl, st));
        else HIPCHK(launch_tail_walk(a, (int32_t)lanes, pl, e->d_h.p, e->d_l.p, e->d_c.p, e->grid, st));
        if (recs)
            HIPCHK(hipMemcpyAsync(recs + i0 * P, a.rec, lanes * sizeof(bt_tail_rec), hipMemcpyDeviceToHost, st));
        if (q)
            HIPCHK(hipMemcpyAsync(q + i0 * P * (size_t)Q, a.q, lanes * (size_t)Q * sizeof(bt_tail_q), hipMemcpyDeviceToHost,
                                  st));
        HIPCHK(hipStreamSynchronize(st));
    });
    return 0;
}

int32_t tail_impl(bt_engine* e, int32_t n, const bt_lane* lanes, int32_t from_bar, int32_t to_bar, int32_t mode, int32_t Q,
                  const int32_t* alpha_ppm, bt_tail_rec* recs, bt_tail_q* q) {
    const char* fn = "bt_tail";
    if (!e) refuse(fn, "null engine");
    const std::string why = tail_refusal(!e->syms.empty(), n, lanes != nullptr, from_bar, to_bar, mode, Q, alpha_ppm,
                                         recs != nullptr, q != nullptr, e->max_bars);
    if (!why.empty()) refuse(fn, why);
    const int32_t to = from_bar == 0 && to_bar == 0 ? INT32_MAX : to_bar;
    if (lanes) {
        int32_t W = 0;
        const std::vector<LaneRef> req = resolve(e, fn, n, lanes, W);
        return tail_run(e, fn, n, &req, nullptr, tail_longest(from_bar, to_bar, W), from_bar, to, mode, Q, alpha_ppm, recs, q);
    }
    return tail_run(e, fn, (int32_t)e->syms.size(), nullptr, nullptr, tail_longest(from_bar, to_bar, e->max_bars), from_bar,
                    to, mode, Q, alpha_ppm, recs, q);
}

int32_t tail_of_impl(bt_engine* e, int32_t n, int32_t T, const int32_t* d, int32_t Q, const int32_t* alpha_ppm,
                     bt_tail_rec* recs, bt_tail_q* q) {
    const char* fn = "bt_tail_of";
    if (!e) refuse(fn, "null engine");
    std::string why = tail_of_refusal(n, T, d != nullptr, Q, alpha_ppm, recs != nullptr, q != nullptr);
    if (why.empty()) why = increments_domain_refusal(n, T, d);
    if (!why.empty()) refuse(fn, why);
    return tail_run(e, fn, n, nullptr, d, T, 0, T, BT_TAIL_ALL, Q, alpha_ppm, recs, q);
}

int32_t last_tail_row_impl(bt_engine* e) {
    if (!e) refuse("bt_last_tail_row", "null engine");
    return e->last_tail_row;
}

// ---- bt_bootstrap / bt_bootstrap_of: the bootstrap reality check (k_boot.hip)
// The start table and vmax are made once; the lanes go through the lane kernel in the chunks of the
// BootPlan (one chunk unless the prefix rows live in the arena or increments are staged); the
// finish reads every lane's record, which stay in the arena for the whole call, and one copy per
// output brings the results back.
struct BootOut {
    bt_boot_group* groups;
    bt_boot_lane* lanes;
    int64_t* vmax;
    int64_t* boot;
};

// `req`: the resolved lanes of a list call; `d`: the increments of a staged call; neither: every
// lane of the dataset, one group per row. `goff`: the groups of a list or staged call, NULL for
// all their lanes as one group.
int32_t boot_run(bt_engine* e, const char* fn, int64_t n, int64_t G, const int32_t* goff, const std::vector<LaneRef>* req,
                 const int32_t* d, int32_t from, int32_t T, int32_t B, int32_t L, uint64_t seed, const BootOut& out) {
    const bool list = req != nullptr, staged = d != nullptr;
    const int32_t one[2] = {0, (int32_t)n};
    if ((list || staged) && !goff) goff = one, G = 1;
    const BootPlan pl = plan_boot(n, G, T, B, L, list, staged, out.boot != nullptr, e->cus, e->boot_row, e->boot_budget);
    std::string why;
    if (pl.row_refused) why = boot_row_refusal(T, ((size_t)T + 1) * 8, kBootLdsBytes - kBootRedBytes);
    if (why.empty()) why = boot_budget_refusal(pl.need_bytes, e->boot_budget > 0 ? (size_t)e->boot_budget : kBootBudget);
    if (!why.empty()) refuse(fn, why);
    std::vector<int32_t> gid;
    if (list || staged) {
        gid.resize((size_t)n);
        for (int64_t g = 0; g < G; ++g)
            for (int32_t i = goff[g]; i < goff[g + 1]; ++i) gid[(size_t)i] = (int32_t)g;
    }
    uint8_t* base = enter(e, pl.staging_bytes);
    hipStream_t st = main_stream(e);
    BootArgs a{};
    a.syms = e->d_syms.p;
    a.lanes = list ? at<const LaneRef>(base, pl.o_lanes) : nullptr;
    a.gid = list || staged ? at<const int32_t>(base, pl.o_gid) : nullptr;
    a.d = staged ? at<const int32_t>(base, pl.o_d) : nullptr;
    a.starts = at<const int32_t>(base, pl.o_starts);
    a.rows = pl.row_mode == 2 ? at<int64_t>(base, pl.o_rows) : nullptr;
    a.vmax = at<int64_t>(base, pl.o_vmax);
    a.boot = out.boot ? at<int64_t>(base, pl.o_boot) : nullptr;
    a.rec = at<bt_boot_lane>(base, pl.o_rec);
    a.goff = list || staged ? at<const int32_t>(base, pl.o_goff) : nullptr;
    a.groups = at<bt_boot_group>(base, pl.o_groups);
    a.pitch = pl.pitch, a.d_pitch = pl.d_pitch;
    a.P = list || staged ? 1 : e->P;
    a.G = (int32_t)G;
    a.from = from, a.T = T, a.B = B, a.Lp = pl.Lp, a.K = pl.K, a.last_len = pl.last_len;
    if (list || staged) {
        HIPCHK(hipMemcpyAsync(base + pl.o_goff, goff, ((size_t)G + 1) * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(base + pl.o_gid, gid.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    }
    if (list) HIPCHK(hipMemcpyAsync(base + pl.o_lanes, req->data(), (size_t)n * sizeof(LaneRef), hipMemcpyHostToDevice, st));
    HIPCHK(launch_boot_starts(a, pl, seed, st));
    for_chunks((size_t)n, (size_t)pl.per_chunk, [&](size_t i0, size_t m) {
        a.lane0 = (int64_t)i0;
        if (staged) {
            HIPCHK(hipMemcpy2DAsync(base + pl.o_d, (size_t)pl.d_pitch * 4, d + i0 * (size_t)T, (size_t)T * 4, (size_t)T * 4,
                                    m, hipMemcpyHostToDevice, st));
            HIPCHK(launch_boot_prefix(a, (int32_t)m, pl, st));   // the next upload is ordered behind it
        } else {
            HIPCHK(launch_boot_walk(a, (int32_t)m, pl, e->d_h.p, e->d_l.p, e->d_c.p, e->grid, st));
        }
    });
    if (out.groups) {
        HIPCHK(launch_boot_finish(a, pl, st));
        HIPCHK(hipMemcpyAsync(out.groups, a.groups, (size_t)G * sizeof(bt_boot_group), hipMemcpyDeviceToHost, st));
    }
    if (out.lanes) HIPCHK(hipMemcpyAsync(out.lanes, a.rec, (size_t)n * sizeof(bt_boot_lane), hipMemcpyDeviceToHost, st));
    if (out.vmax) HIPCHK(hipMemcpyAsync(out.vmax, a.vmax, (size_t)G * (size_t)B * 8, hipMemcpyDeviceToHost, st));
    if (out.boot) HIPCHK(hipMemcpyAsync(out.boot, a.boot, (size_t)n * (size_t)B * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

int32_t bootstrap_impl(bt_engine* e, int32_t n, const bt_lane* lanes, int32_t G, const int32_t* goff, int32_t from_bar,
                       int32_t to_bar, int32_t B, int32_t L, uint64_t seed, const BootOut& out) {
    const char* fn = "bt_bootstrap";
    const BootCall call{e != nullptr, e && !e->syms.empty(), false, lanes != nullptr, n, G, goff, from_bar, to_bar, B, L,
                        out.groups || out.lanes || out.vmax || out.boot, out.boot != nullptr};
    std::string why = boot_refusal(call);
    if (!why.empty()) refuse(fn, why);
    int32_t T = 0;
    if (lanes) {
        int32_t W = 0;
        const std::vector<LaneRef> req = resolve(e, fn, n, lanes, W);
        why = boot_window(from_bar, to_bar, W, T);
        if (!why.empty()) refuse(fn, why);
        return boot_run(e, fn, n, G, goff, &req, nullptr, from_bar, T, B, L, seed, out);
    }
    why = boot_window(from_bar, to_bar, e->max_bars, T);
    if (!why.empty()) refuse(fn, why);
    const int64_t S = (int64_t)e->syms.size();
    return boot_run(e, fn, S * e->P, S, nullptr, nullptr, nullptr, from_bar, T, B, L, seed, out);
}

int32_t bootstrap_of_impl(bt_engine* e, int32_t n, int32_t T, const int32_t* d, int32_t G, const int32_t* goff, int32_t B,
                          int32_t L, uint64_t seed, const BootOut& out) {
    const char* fn = "bt_bootstrap_of";
    const BootCall call{e != nullptr, false, true, d != nullptr, n, G, goff, 0, T, B, L,
                        out.groups || out.lanes || out.vmax || out.boot, out.boot != nullptr};
    // T before the rest: a row without bars has no d to ask for
    int32_t Tw = 0;
    std::string why = e ? boot_window(0, T, 0, Tw) : "";
    if (why.empty()) why = boot_refusal(call);
    if (!why.empty()) refuse(fn, why);
    why = increments_domain_refusal(n, T, d);
    if (!why.empty()) refuse(fn, why);
    return boot_run(e, fn, n, G, goff, nullptr, d, 0, T, B, L, seed, out);
}

// ---- bt_drawdown_boot / bt_drawdown_boot_of: the bootstrap of every lane's largest drawdown (k_ddboot.hip)
// The start table (the reality check's kernel), the levels and the limits are made once; the lanes go
// through the lane kernel in the chunks of the DdPlan, and every chunk brings its own results back.
struct DdOut {
    bt_dd_lane* rec;
    int64_t* q;
    int64_t* reach;
    int64_t* raw;
};

// `req`: the resolved lanes of a list call; `d`: the increments of a staged call; neither: every
// lane of the dataset.
int32_t dd_run(bt_engine* e, const char* fn, int64_t n, const std::vector<LaneRef>* req, const int32_t* d, int32_t from,
               int32_t T, int32_t B, int32_t L, uint64_t seed, int32_t Q, const int32_t* alpha_ppm, int32_t R,
               const int64_t* limits, DdOut out) {
    const bool list = req != nullptr, staged = d != nullptr;
    if (Q == 0) out.q = nullptr;
    if (R == 0) out.reach = nullptr;
    if (!out.q) Q = 0;               // levels nobody reads are not selected
    if (!out.reach) R = 0;
    const DdPlan pl = plan_ddboot(n, T, B, L, Q, R, list, staged, out.raw != nullptr, e->cus, e->ddboot_row, e->ddboot_budget);
    std::string why;
    if (pl.row_refused) why = dd_row_refusal(T, pl.row_bytes, kDdLdsBytes - kDdFixedBytes);
    if (why.empty()) why = dd_budget_refusal(pl.need_bytes, e->ddboot_budget > 0 ? (size_t)e->ddboot_budget : kDdBudget);
    if (!why.empty()) refuse(fn, why);
    uint8_t* base = enter(e, pl.staging_bytes);
    hipStream_t st = main_stream(e);
    e->last_ddboot_row = pl.row_mode;
    DdArgs a{};
    a.syms = e->d_syms.p;
    a.lanes = list ? at<const LaneRef>(base, pl.o_lanes) : nullptr;
    a.d = staged ? at<const int32_t>(base, pl.o_d) : nullptr;
    a.starts = at<const int32_t>(base, pl.o_starts);
    a.levels = at<const int32_t>(base, pl.o_levels);
    a.limits = at<const int64_t>(base, pl.o_limits);
    a.rows = pl.row_mode == 2 ? base + pl.o_rows : nullptr;
    a.vals = pl.v_pitch > 0 ? at<int64_t>(base, pl.o_vals) : nullptr;
    a.raw = out.raw ? at<int64_t>(base, pl.o_raw) : nullptr;
    a.rec = out.rec ? at<bt_dd_lane>(base, pl.o_rec) : nullptr;
    a.q = out.q ? at<int64_t>(base, pl.o_q) : nullptr;
    a.reach = out.reach ? at<int64_t>(base, pl.o_reach) : nullptr;
    a.pitch = pl.pitch, a.d_pitch = pl.d_pitch, a.v_pitch = pl.v_pitch;
    a.r_w1 = (uint32_t)pl.r_w1, a.r_w2 = (uint32_t)pl.r_w2, a.l_vals = (uint32_t)pl.l_vals;
    a.P = list || staged ? 1 : e->P;
    a.from = from, a.T = T, a.B = B, a.Lp = pl.Lp, a.K = pl.K, a.last_len = pl.last_len, a.Q = Q, a.R = R;
    if (Q > 0) HIPCHK(hipMemcpyAsync(base + pl.o_levels, alpha_ppm, (size_t)Q * 4, hipMemcpyHostToDevice, st));
    if (R > 0) HIPCHK(hipMemcpyAsync(base + pl.o_limits, limits, (size_t)R * 8, hipMemcpyHostToDevice, st));
    // the reality check's start kernel, with no group: it writes the table alone
    BootArgs sa{};
    sa.starts = a.starts;
    sa.T = T, sa.B = B, sa.K = pl.K;
    BootPlan sp{};
    sp.starts_block = pl.starts_block, sp.starts_blocks = pl.starts_blocks;
    HIPCHK(launch_boot_starts(sa, sp, seed, st));
    HIPCHK(prepare_dd(pl, staged, e->grid));
    for_chunks((size_t)n, (size_t)pl.per_chunk, [&](size_t i0, size_t m) {
        a.lane0 = (int64_t)i0;
        if (list) HIPCHK(hipMemcpyAsync(base + pl.o_lanes, req->data() + i0, m * sizeof(LaneRef), hipMemcpyHostToDevice, st));
        if (staged) {
            HIPCHK(hipMemcpy2DAsync(base + pl.o_d, (size_t)pl.d_pitch * 4, d + i0 * (size_t)T, (size_t)T * 4, (size_t)T * 4,
                                    m, hipMemcpyHostToDevice, st));
            HIPCHK(launch_dd_of(a, (int32_t)m, pl, st));
        } else {
            HIPCHK(launch_dd_walk(a, (int32_t)m, pl, e->d_h.p, e->d_l.p, e->d_c.p, e->grid, st));
        }
        if (out.rec) HIPCHK(hipMemcpyAsync(out.rec + i0, a.rec, m * sizeof(bt_dd_lane), hipMemcpyDeviceToHost, st));
        if (out.q) HIPCHK(hipMemcpyAsync(out.q + i0 * (size_t)Q, a.q, m * (size_t)Q * 8, hipMemcpyDeviceToHost, st));
        if (out.reach)
            HIPCHK(hipMemcpyAsync(out.reach + i0 * (size_t)R, a.reach, m * (size_t)R * 8, hipMemcpyDeviceToHost, st));
        if (out.raw) HIPCHK(hipMemcpyAsync(out.raw + i0 * (size_t)B, a.raw, m * (size_t)B * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    });
    return 0;
}

int32_t drawdown_boot_impl(bt_engine* e, int32_t n, const bt_lane* lanes, int32_t from_bar, int32_t to_bar, int32_t B,
                           int32_t L, uint64_t seed, int32_t Q, const int32_t* alpha_ppm, int32_t R, const int64_t* limits,
                           const DdOut& out) {
    const char* fn = "bt_drawdown_boot";
    const DdCall call{e != nullptr, e && !e->syms.empty(), false, lanes != nullptr, n, from_bar, B, L, Q, alpha_ppm, R, limits,
                      out.rec != nullptr, out.q != nullptr, out.reach != nullptr, out.raw != nullptr};
    std::string why = dd_refusal(call);
    if (!why.empty()) refuse(fn, why);
    int32_t T = 0;
    if (lanes) {
        int32_t W = 0;
        const std::vector<LaneRef> req = resolve(e, fn, n, lanes, W);
        why = boot_window(from_bar, to_bar, W, T);
        if (!why.empty()) refuse(fn, why);
        return dd_run(e, fn, n, &req, nullptr, from_bar, T, B, L, seed, Q, alpha_ppm, R, limits, out);
    }
    why = boot_window(from_bar, to_bar, e->max_bars, T);
    if (!why.empty()) refuse(fn, why);
    return dd_run(e, fn, (int64_t)e->syms.size() * e->P, nullptr, nullptr, from_bar, T, B, L, seed, Q, alpha_ppm, R, limits,
                  out);
}

int32_t drawdown_boot_of_impl(bt_engine* e, int32_t n, int32_t T, const int32_t* d, int32_t B, int32_t L, uint64_t seed,
                              int32_t Q, const int32_t* alpha_ppm, int32_t R, const int64_t* limits, const DdOut& out) {
    const char* fn = "bt_drawdown_boot_of";
    const DdCall call{e != nullptr, false, true, d != nullptr, n, 0, B, L, Q, alpha_ppm, R, limits,
                      out.rec != nullptr, out.q != nullptr, out.reach != nullptr, out.raw != nullptr};
    // T before the rest: a row without bars has no d to ask for
    int32_t Tw = 0;
    std::string why = e ? boot_window(0, T, 0, Tw) : "";
    if (why.empty()) why = dd_refusal(call);
    if (!why.empty()) refuse(fn, why);
    why = increments_domain_refusal(n, T, d);
    if (!why.empty()) refuse(fn, why);
    return dd_run(e, fn, n, nullptr, d, 0, T, B, L, seed, Q, alpha_ppm, R, limits, out);
}

int32_t last_ddboot_row_impl(bt_engine* e) {
    if (!e) refuse("bt_last_ddboot_row", "null engine");
    return e->last_ddboot_row;
}

// ---- bt_portfolio: chosen lanes traded together, per bar (k_portfolio.hip)
// The entries with a non-empty window go up once, the accumulators are zeroed, the walk adds into
// them and the finish writes the four rows and the summary, which one copy brings back.
int32_t portfolio_impl(bt_engine* e, int32_t n, const bt_pf_lane* lanes, int32_t T, int64_t* pnl, int64_t* equity,
                       int32_t* n_long, int32_t* n_short, bt_pf_summary* summary) {
    const char* fn = "bt_portfolio";
    if (!e) refuse(fn, "null engine");
    std::string why = portfolio_refusal(!e->syms.empty(), n, lanes != nullptr, T,
                                        pnl || equity || n_long || n_short || summary);
    if (!why.empty()) refuse(fn, why);
    PfResolved rs;
    why = portfolio_resolve(e->syms.data(), e->syms.size(), e->P, n, lanes, T, rs);
    if (!why.empty()) refuse(fn, why);
    const int32_t m = (int32_t)rs.req.size();
    const PortfolioPlan pl = plan_portfolio(m, T, e->cus, e->portfolio_replicas);
    uint8_t* base = enter(e, pl.staging_bytes);
    e->h_portfolio.ensure(pl.out_bytes);
    PfLane* d_lanes = at<PfLane>(base, pl.o_lanes);
    PfWork w{};
    w.acc_pnl = at<unsigned long long>(base, pl.o_acc_pnl);
    w.acc_cnt = at<unsigned long long>(base, pl.o_acc_cnt);
    w.pitch = pl.pitch;
    w.R = pl.R;
    w.T = T;
    w.n_lanes = rs.n_lanes, w.lo = rs.lo, w.hi = rs.hi;
    w.pnl = at<int64_t>(base, pl.o_pnl);
    w.equity = at<int64_t>(base, pl.o_equity);
    w.n_long = at<int32_t>(base, pl.o_long);
    w.n_short = at<int32_t>(base, pl.o_short);
    w.sum = at<bt_pf_summary>(base, pl.o_sum);
    if (m > 0)
        HIPCHK(hipMemcpyAsync(d_lanes, rs.req.data(), (size_t)m * sizeof(PfLane), hipMemcpyHostToDevice, main_stream(e)));
    HIPCHK(hipMemsetAsync(base + pl.o_acc_pnl, 0, pl.acc_bytes, main_stream(e)));
    HIPCHK(launch_portfolio(d_lanes, m, e->d_h.p, e->d_l.p, e->d_c.p, e->grid, w, pl, main_stream(e)));
    HIPCHK(hipMemcpyAsync(e->h_portfolio.p, base + pl.o_pnl, pl.out_bytes, hipMemcpyDeviceToHost, main_stream(e)));
    HIPCHK(hipStreamSynchronize(main_stream(e)));
    const uint8_t* h = e->h_portfolio.p;
    const size_t bars = (size_t)T;
    if (pnl) memcpy(pnl, h, bars * 8);
    if (equity) memcpy(equity, h + (pl.o_equity - pl.o_pnl), bars * 8);
    if (n_long) memcpy(n_long, h + (pl.o_long - pl.o_pnl), bars * 4);
    if (n_short) memcpy(n_short, h + (pl.o_short - pl.o_pnl), bars * 4);
    if (summary) memcpy(summary, h + (pl.o_sum - pl.o_pnl), sizeof *summary);
    return 0;
}

// ---- bt_covariance / bt_gram_of: the exact Gram matrix of per-bar increments (k_gram.hip)
// D is zeroed, filled (by the walk, or by the caller's rows), multiplied and folded; one copy
// brings gram and sums back.
GramWork gram_work(uint8_t* base, const GramPlan& pl, int32_t n, int32_t T) {
    GramWork w{};
    w.D = at<int32_t>(base, pl.o_d);
    w.pitch = pl.pitch;
    w.partial = at<bt_wide>(base, pl.o_partial);
    w.gram = at<bt_wide>(base, pl.o_gram);
    w.sums = at<int64_t>(base, pl.o_sums);
    w.n = n, w.T = T;
    w.nt = pl.nt, w.tiles = pl.tiles;
    w.chunks = pl.chunks, w.chunk_bars = pl.chunk_bars;
    return w;
}

void gram_fetch(bt_engine* e, uint8_t* base, const GramPlan& pl, int32_t n, bt_wide* gram, int64_t* sums) {
    e->h_gram.ensure(pl.out_bytes);
    HIPCHK(hipMemcpyAsync(e->h_gram.p, base + pl.o_gram, pl.out_bytes, hipMemcpyDeviceToHost, main_stream(e)));
    HIPCHK(hipStreamSynchronize(main_stream(e)));
    if (gram) memcpy(gram, e->h_gram.p, (size_t)n * (size_t)n * sizeof(bt_wide));
    if (sums) memcpy(sums, e->h_gram.p + (pl.o_sums - pl.o_gram), (size_t)n * sizeof(int64_t));
}

int32_t covariance_impl(bt_engine* e, int32_t n, const bt_lane* lanes, int32_t from_bar, int32_t to_bar,
                        bt_wide* gram, int64_t* sums, int32_t* T_out) {
    const char* fn = "bt_covariance";
    if (!e) refuse(fn, "null engine");
    std::string why = covariance_refusal(!e->syms.empty(), n, lanes != nullptr, from_bar, to_bar, gram || sums || T_out);
    if (!why.empty()) refuse(fn, why);
    int32_t W = 0, T = 0;
    const std::vector<LaneRef> req = resolve(e, fn, n, lanes, W);
    why = covariance_window(from_bar, to_bar, W, T);
    if (!why.empty()) refuse(fn, why);
    const GramPlan pl = plan_gram(n, T, e->cus, e->gram_split);
    why = gram_staging_refusal(pl.staging_bytes, kGramStagingMax, n, T);
    if (!why.empty()) refuse(fn, why);
    if (T_out) *T_out = T;
    if (n == 0 || T == 0) {
        if (gram) memset(gram, 0, (size_t)n * (size_t)n * sizeof(bt_wide));
        if (sums) memset(sums, 0, (size_t)n * sizeof(int64_t));
        return 0;
    }
    uint8_t* base = enter(e, pl.staging_bytes);
    LaneRef* d_lanes = at<LaneRef>(base, pl.o_lanes);
    const GramWork w = gram_work(base, pl, n, T);
    HIPCHK(hipMemcpyAsync(d_lanes, req.data(), (size_t)n * sizeof(LaneRef), hipMemcpyHostToDevice, main_stream(e)));
    HIPCHK(hipMemsetAsync(base + pl.o_d, 0, pl.d_bytes, main_stream(e)));
    HIPCHK(launch_gram_walk(d_lanes, e->d_h.p, e->d_l.p, e->d_c.p, e->grid, w, from_bar, from_bar + T, main_stream(e)));
    HIPCHK(launch_gram(w, pl, false, main_stream(e)));
    gram_fetch(e, base, pl, n, gram, sums);
    return 0;
}

int32_t gram_of_impl(bt_engine* e, int32_t n, int32_t T, const int32_t* d, bt_wide* gram, int64_t* sums) {
    const char* fn = "bt_gram_of";
    if (!e) refuse(fn, "null engine");
    std::string why = gram_of_refusal(n, T, d != nullptr, gram || sums);
    if (!why.empty()) refuse(fn, why);
    const GramPlan pl = plan_gram(n, T, e->cus, e->gram_split);
    why = gram_staging_refusal(pl.staging_bytes, kGramStagingMax, n, T);
    if (!why.empty()) refuse(fn, why);
    if (n == 0 || T == 0) {
        if (gram) memset(gram, 0, (size_t)n * (size_t)n * sizeof(bt_wide));
        if (sums) memset(sums, 0, (size_t)n * sizeof(int64_t));
        return 0;
    }
    why = increments_domain_refusal(n, T, d);
    if (!why.empty()) refuse(fn, why);
    uint8_t* base = enter(e, pl.staging_bytes);
    const GramWork w = gram_work(base, pl, n, T);
    HIPCHK(hipMemsetAsync(base + pl.o_d, 0, pl.d_bytes, main_stream(e)));
    HIPCHK(hipMemcpy2DAsync(w.D, (size_t)pl.pitch * sizeof(int32_t), d, (size_t)T * sizeof(int32_t),
                            (size_t)T * sizeof(int32_t), (size_t)n, hipMemcpyHostToDevice, main_stream(e)));
    HIPCHK(launch_gram(w, pl, true, main_stream(e)));
    gram_fetch(e, base, pl, n, gram, sums);
    return 0;
}

}  // namespace

extern "C" {

int32_t bt_covariance(bt_engine* e, int32_t n, const bt_lane* lanes, int32_t from_bar, int32_t to_bar, bt_wide* gram,
                      int64_t* sums, int32_t* T_out) {
    ABI_GUARD(-1, { return covariance_impl(e, n, lanes, from_bar, to_bar, gram, sums, T_out); })
}

int32_t bt_gram_of(bt_engine* e, int32_t n, int32_t T, const int32_t* d, bt_wide* gram, int64_t* sums) {
    ABI_GUARD(-1, { return gram_of_impl(e, n, T, d, gram, sums); })
}

int32_t bt_set_gram_split(bt_engine* e, int32_t k) {
    ABI_GUARD(-1, { return set_knob(e, "bt_set_gram_split", "k", k, -1, &EngineState::gram_split); })
}

int32_t bt_portfolio(bt_engine* e, int32_t n, const bt_pf_lane* lanes, int32_t T, int64_t* pnl, int64_t* equity,
                     int32_t* n_long, int32_t* n_short, bt_pf_summary* summary) {
    ABI_GUARD(-1, { return portfolio_impl(e, n, lanes, T, pnl, equity, n_long, n_short, summary); })
}

int32_t bt_set_portfolio_replicas(bt_engine* e, int32_t r) {
    ABI_GUARD(-1, { return set_knob(e, "bt_set_portfolio_replicas", "r", r, -1, &EngineState::portfolio_replicas); })
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

int32_t bt_topk_of(bt_engine* e, int32_t S, int32_t P, const bt_summary* sum, const int32_t* sym_ids, int32_t k,
                   int32_t lds_free_hist, bt_topk_rec* out) {
    ABI_GUARD(-1, { return topk_of_impl(e, S, P, sum, sym_ids, k, lds_free_hist, out); })
}

int32_t bt_walk_forward(bt_engine* e, int32_t K, const int32_t* bounds, int32_t train, bt_fold* folds,
                        bt_wf_step* steps, bt_fold* total) {
    ABI_GUARD(-1, { return walk_forward_impl(e, K, bounds, train, folds, steps, total); })
}

int32_t bt_set_walkfwd_budget(bt_engine* e, int64_t bytes) {
    ABI_GUARD(-1, { return set_knob(e, "bt_set_walkfwd_budget", "bytes", bytes, -1, &EngineState::walkfwd_budget); })
}

int32_t bt_cscv(bt_engine* e, int32_t K, const int32_t* bounds, bt_cscv_group* groups, uint32_t* hist,
                bt_cscv_pick* picks) {
    ABI_GUARD(-1, { return cscv_impl(e, K, bounds, groups, hist, picks); })
}

int32_t bt_cscv_of(bt_engine* e, int32_t G, int32_t P, int32_t K, const bt_fold* folds, const int32_t* sym_ids,
                   bt_cscv_group* groups, uint32_t* hist, bt_cscv_pick* picks) {
    ABI_GUARD(-1, { return cscv_of_impl(e, G, P, K, folds, sym_ids, groups, hist, picks); })
}

int32_t bt_set_cscv_work(bt_engine* e, int64_t cells) {
    ABI_GUARD(-1, { return set_knob(e, "bt_set_cscv_work", "cells", cells, -1, &EngineState::cscv_work); })
}

int32_t bt_trade_stats(bt_engine* e, int32_t n, const bt_lane* lanes, bt_tstats* out, bt_tstats_agg* agg) {
    ABI_GUARD(-1, { return trade_stats_impl(e, n, lanes, out, agg); })
}

int32_t bt_set_tstats_budget(bt_engine* e, int64_t bytes) {
    ABI_GUARD(-1, { return set_knob(e, "bt_set_tstats_budget", "bytes", bytes, -1, &EngineState::tstats_budget); })
}

int32_t bt_costs(bt_engine* e, int32_t C, const int32_t* levels, int32_t n, const bt_lane* lanes, bt_cost_rec* out,
                 bt_cost_agg* agg) {
    ABI_GUARD(-1, { return costs_impl(e, C, levels, n, lanes, out, agg); })
}

int32_t bt_set_costs_budget(bt_engine* e, int64_t bytes) {
    ABI_GUARD(-1, { return set_knob(e, "bt_set_costs_budget", "bytes", bytes, -1, &EngineState::costs_budget); })
}

int32_t bt_tail(bt_engine* e, int32_t n, const bt_lane* lanes, int32_t from_bar, int32_t to_bar, int32_t mode, int32_t Q,
                const int32_t* alpha_ppm, bt_tail_rec* recs_out, bt_tail_q* q_out) {
    ABI_GUARD(-1, { return tail_impl(e, n, lanes, from_bar, to_bar, mode, Q, alpha_ppm, recs_out, q_out); })
}

int32_t bt_tail_of(bt_engine* e, int32_t n, int32_t T, const int32_t* d, int32_t Q, const int32_t* alpha_ppm,
                   bt_tail_rec* recs_out, bt_tail_q* q_out) {
    ABI_GUARD(-1, { return tail_of_impl(e, n, T, d, Q, alpha_ppm, recs_out, q_out); })
}

int32_t bt_set_tail_row(bt_engine* e, int32_t mode) {
    ABI_GUARD(-1, { return set_knob(e, "bt_set_tail_row", "mode", mode, 2, &EngineState::tail_row); })
}

int32_t bt_set_tail_budget(bt_engine* e, int64_t bytes) {
    ABI_GUARD(-1, { return set_knob(e, "bt_set_tail_budget", "bytes", bytes, -1, &EngineState::tail_budget); })
}

int32_t bt_last_tail_row(bt_engine* e) {
    ABI_GUARD(-1, { return last_tail_row_impl(e); })
}

int32_t bt_bootstrap(bt_engine* e, int32_t n, const bt_lane* lanes, int32_t G, const int32_t* goff, int32_t from_bar,
                     int32_t to_bar, int32_t B, int32_t L, uint64_t seed, bt_boot_group* groups_out,
                     bt_boot_lane* lanes_out, int64_t* vmax_out, int64_t* boot_out) {
    ABI_GUARD(-1, {
        return bootstrap_impl(e, n, lanes, G, goff, from_bar, to_bar, B, L, seed,
                              BootOut{groups_out, lanes_out, vmax_out, boot_out});
    })
}

int32_t bt_bootstrap_of(bt_engine* e, int32_t n, int32_t T, const int32_t* d, int32_t G, const int32_t* goff,
                        int32_t B, int32_t L, uint64_t seed, bt_boot_group* groups_out, bt_boot_lane* lanes_out,
                        int64_t* vmax_out, int64_t* boot_out) {
    ABI_GUARD(-1, {
        return bootstrap_of_impl(e, n, T, d, G, goff, B, L, seed, BootOut{groups_out, lanes_out, vmax_out, boot_out});
    })
}

int32_t bt_set_boot_budget(bt_engine* e, int64_t bytes) {
    ABI_GUARD(-1, { return set_knob(e, "bt_set_boot_budget", "bytes", bytes, -1, &EngineState::boot_budget); })
}

int32_t bt_set_boot_row(bt_engine* e, int32_t mode) {
    ABI_GUARD(-1, { return set_knob(e, "bt_set_boot_row", "mode", mode, 2, &EngineState::boot_row); })
}

int32_t bt_drawdown_boot(bt_engine* e, int32_t n, const bt_lane* lanes, int32_t from_bar, int32_t to_bar, int32_t B,
                         int32_t L, uint64_t seed, int32_t Q, const int32_t* alpha_ppm, int32_t R, const int64_t* limits,
                         bt_dd_lane* lanes_out, int64_t* q_out, int64_t* reach_out, int64_t* raw_out) {
    ABI_GUARD(-1, {
        return drawdown_boot_impl(e, n, lanes, from_bar, to_bar, B, L, seed, Q, alpha_ppm, R, limits,
                                  DdOut{lanes_out, q_out, reach_out, raw_out});
    })
}

int32_t bt_drawdown_boot_of(bt_engine* e, int32_t n, int32_t T, const int32_t* d, int32_t B, int32_t L, uint64_t seed,
                            int32_t Q, const int32_t* alpha_ppm, int32_t R, const int64_t* limits, bt_dd_lane* lanes_out,
                            int64_t* q_out, int64_t* reach_out, int64_t* raw_out) {
    ABI_GUARD(-1, {
        return drawdown_boot_of_impl(e, n, T, d, B, L, seed, Q, alpha_ppm, R, limits,
                                     DdOut{lanes_out, q_out, reach_out, raw_out});
    })
}

int32_t bt_set_ddboot_budget(bt_engine* e, int64_t bytes) {
    ABI_GUARD(-1, { return set_knob(e, "bt_set_ddboot_budget", "bytes", bytes, -1, &EngineState::ddboot_budget); })
}

int32_t bt_set_ddboot_row(bt_engine* e, int32_t mode) {
    ABI_GUARD(-1, { return set_knob(e, "bt_set_ddboot_row", "mode", mode, 2, &EngineState::ddboot_row); })
}

int32_t bt_last_ddboot_row(bt_engine* e) {
    ABI_GUARD(-1, { return last_ddboot_row_impl(e); })
}

int32_t bt_set_surface_chunks(bt_engine* e, int32_t chunks) {
    ABI_GUARD(-1, { return set_knob(e, "bt_set_surface_chunks", "chunks", chunks, -1, &EngineState::surface_chunks); })
}

}  // extern "C"
