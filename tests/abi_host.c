/* abi_host.c — a compiled C99 host of the drop-in boundary (include/bt.h), the way the Rust
 * worker's process_incoming_job would drive it (the reference's job loop is
 * /root/reference/src/worker/process.rs:13-29): create an engine, one bt_run_batch per JobsReply,
 * free the library-owned strings, destroy. Test support only (tests/test_abi_cpu.py compiles it
 * with -std=c99 -pedantic -Werror and checks the struct layouts against the ctypes mirror;
 * tests/test_gpu_parity.py runs a batch through it and compares with the Python host).
 *
 *   abi_host layout                      struct sizes and field offsets as JSON (no GPU)
 *   abi_host run SEED N BARS              N synthetic daily jobs (DBXCOL1 payloads) as one batch;
 *                                        prints "== job i status s len n" and the data per job
 */
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bt.h"

#define OFF(T, f) printf("\"%s.%s\": %zu, ", #T, #f, offsetof(T, f))
#define SZ(T) printf("\"%s\": %zu, ", #T, sizeof(T))

/* Every record the Python mirror keeps as a numpy dtype (records.py RECORDS): its size and the
 * offset of every field, under the names the mirror uses (OFFN: bt_boot_lane's m1 and m2 lie flat
 * there). */
#define OFFN(T, name, f) printf("\"%s.%s\": %zu, ", #T, #name, offsetof(T, f))
static void records(void) {
    SZ(bt_summary); OFF(bt_summary, n_trades); OFF(bt_summary, status); OFF(bt_summary, pnl);
    OFF(bt_summary, mdd); OFF(bt_summary, exposure); OFF(bt_summary, sharpe); OFF(bt_summary, hash);
    SZ(bt_trade); OFF(bt_trade, entry_bar); OFF(bt_trade, exit_bar); OFF(bt_trade, side);
    OFF(bt_trade, pad); OFF(bt_trade, entry_px); OFF(bt_trade, exit_px);
    SZ(bt_sums); OFF(bt_sums, s1_lo); OFF(bt_sums, s1_hi); OFF(bt_sums, s2_lo); OFF(bt_sums, s2_hi);
    SZ(bt_topk_rec); OFF(bt_topk_rec, sharpe); OFF(bt_topk_rec, sym); OFF(bt_topk_rec, param);
    OFF(bt_topk_rec, pnl);
    SZ(bt_lane); OFF(bt_lane, sym); OFF(bt_lane, param);
    SZ(bt_param_agg); OFF(bt_param_agg, n_sym); OFF(bt_param_agg, n_traded);
    OFF(bt_param_agg, n_win); OFF(bt_param_agg, n_pos); OFF(bt_param_agg, trades);
    OFF(bt_param_agg, pnl); OFF(bt_param_agg, exposure); OFF(bt_param_agg, mdd_max);
    OFF(bt_param_agg, sharpe_max); OFF(bt_param_agg, sharpe_min); OFF(bt_param_agg, sym_max);
    OFF(bt_param_agg, sym_min); OFF(bt_param_agg, ss1_lo); OFF(bt_param_agg, ss1_hi);
    OFF(bt_param_agg, ss2_lo); OFF(bt_param_agg, ss2_hi);
    SZ(bt_fold); OFF(bt_fold, first_bar); OFF(bt_fold, n_bars); OFF(bt_fold, n_trades);
    OFF(bt_fold, status); OFF(bt_fold, pnl); OFF(bt_fold, mdd); OFF(bt_fold, exposure);
    OFF(bt_fold, sharpe); OFF(bt_fold, s1_lo); OFF(bt_fold, s1_hi); OFF(bt_fold, s2_lo);
    OFF(bt_fold, s2_hi);
    SZ(bt_wf_step); OFF(bt_wf_step, sym); OFF(bt_wf_step, fold); OFF(bt_wf_step, param);
    OFF(bt_wf_step, pad); OFF(bt_wf_step, train_sharpe); OFF(bt_wf_step, oos);
    SZ(bt_pf_lane); OFF(bt_pf_lane, sym); OFF(bt_pf_lane, param); OFF(bt_pf_lane, from_bar);
    OFF(bt_pf_lane, to_bar);
    SZ(bt_pf_summary); OFF(bt_pf_summary, n_lanes); OFF(bt_pf_summary, first_bar);
    OFF(bt_pf_summary, n_bars); OFF(bt_pf_summary, max_gross); OFF(bt_pf_summary, pnl);
    OFF(bt_pf_summary, mdd); OFF(bt_pf_summary, exposure); OFF(bt_pf_summary, sharpe);
    OFF(bt_pf_summary, s1_lo); OFF(bt_pf_summary, s1_hi); OFF(bt_pf_summary, s2_lo);
    OFF(bt_pf_summary, s2_hi);
    SZ(bt_wide); OFF(bt_wide, lo); OFF(bt_wide, hi);
    SZ(bt_tstats); OFF(bt_tstats, n_trades); OFF(bt_tstats, n_win); OFF(bt_tstats, n_loss);
    OFF(bt_tstats, status); OFF(bt_tstats, n_long); OFF(bt_tstats, n_long_win);
    OFF(bt_tstats, max_win_streak); OFF(bt_tstats, max_loss_streak); OFF(bt_tstats, hold_sum);
    OFF(bt_tstats, hold_win); OFF(bt_tstats, hold_max); OFF(bt_tstats, n_bars);
    OFF(bt_tstats, gross_win); OFF(bt_tstats, gross_loss); OFF(bt_tstats, max_win);
    OFF(bt_tstats, max_loss); OFF(bt_tstats, sq_lo); OFF(bt_tstats, sq_hi); OFF(bt_tstats, mdd);
    OFF(bt_tstats, mdd_bar); OFF(bt_tstats, peak_bar); OFF(bt_tstats, underwater_bars);
    OFF(bt_tstats, max_underwater); OFF(bt_tstats, hash);
    SZ(bt_tstats_agg); OFF(bt_tstats_agg, n_sym); OFF(bt_tstats_agg, n_traded);
    OFF(bt_tstats_agg, max_win_streak); OFF(bt_tstats_agg, max_loss_streak);
    OFF(bt_tstats_agg, hold_max); OFF(bt_tstats_agg, max_underwater); OFF(bt_tstats_agg, n_trades);
    OFF(bt_tstats_agg, n_win); OFF(bt_tstats_agg, n_loss); OFF(bt_tstats_agg, n_long);
    OFF(bt_tstats_agg, n_long_win); OFF(bt_tstats_agg, hold_sum); OFF(bt_tstats_agg, hold_win);
    OFF(bt_tstats_agg, gross_win); OFF(bt_tstats_agg, gross_loss); OFF(bt_tstats_agg, max_win);
    OFF(bt_tstats_agg, max_loss); OFF(bt_tstats_agg, mdd_max); OFF(bt_tstats_agg, sq_lo);
    OFF(bt_tstats_agg, sq_hi);
    SZ(bt_boot_lane); OFF(bt_boot_lane, sum); OFF(bt_boot_lane, n_nonpos);
    OFFN(bt_boot_lane, m1_lo, m1.lo); OFFN(bt_boot_lane, m1_hi, m1.hi);
    OFFN(bt_boot_lane, m2_lo, m2.lo); OFFN(bt_boot_lane, m2_hi, m2.hi);
    SZ(bt_boot_group); OFF(bt_boot_group, best_sum); OFF(bt_boot_group, best_lane);
    OFF(bt_boot_group, n_lanes); OFF(bt_boot_group, n_ge);
}

static int layout(void) {
    printf("{");
    SZ(bt_config);
    OFF(bt_config, strategy); OFF(bt_config, fast); OFF(bt_config, slow); OFF(bt_config, n_span);
    OFF(bt_config, span); OFF(bt_config, ols); OFF(bt_config, band_bps); OFF(bt_config, n_bwin);
    OFF(bt_config, bwin); OFF(bt_config, k_num); OFF(bt_config, k_den); OFF(bt_config, sl_bps);
    OFF(bt_config, tp_bps); OFF(bt_config, annualization); OFF(bt_config, device);
    OFF(bt_config, topk); OFF(bt_config, flags); OFF(bt_config, host_threads);
    OFF(bt_config, trade_cap); OFF(bt_config, stream);
    SZ(bt_job_in); OFF(bt_job_in, file); OFF(bt_job_in, len);
    SZ(bt_job_out); OFF(bt_job_out, len); OFF(bt_job_out, status); OFF(bt_job_out, n_bars);
    SZ(bt_stats); SZ(bt_batch_profile); OFF(bt_batch_profile, payload_bytes_read);
    OFF(bt_batch_profile, bars); OFF(bt_batch_profile, host_ingest_ms);
    OFF(bt_batch_profile, total_ms);
    records();
    printf("\"abi_version\": %d}\n", (int)bt_abi_version());
    return 0;
}

static int run(uint64_t seed, int n, int bars) {
    static const int32_t fast[] = {4, 6, 10}, slow[] = {50, 60, 120};
    bt_config cfg;
    char err[256];
    bt_engine* e;
    bt_job_in* jobs = calloc((size_t)n, sizeof *jobs);
    bt_job_out* outs = calloc((size_t)n, sizeof *outs);
    uint8_t** bufs = calloc((size_t)n, sizeof *bufs);
    char (*ids)[32] = calloc((size_t)n, sizeof *ids);
    int i, rc = 0;
    if (!jobs || !outs || !bufs || !ids) return 2;
    memset(&cfg, 0, sizeof cfg);
    cfg.strategy = BT_SMA_CROSS;
    cfg.n_fast = 3;
    cfg.n_slow = 3;
    cfg.fast = fast;
    cfg.slow = slow;
    cfg.annualization = 252;
    e = bt_engine_create(&cfg, err, sizeof err);
    if (!e) {
        fprintf(stderr, "bt_engine_create: %s\n", err);
        return 1;
    }
    for (i = 0; i < n; ++i) {
        const int64_t need = bt_gen_payload(seed, i, bars, BT_DAILY, NULL, 0);
        bufs[i] = need > 0 ? malloc((size_t)need) : NULL;
        if (!bufs[i] || bt_gen_payload(seed, i, bars, BT_DAILY, bufs[i], (size_t)need) != need) {
            fprintf(stderr, "bt_gen_payload failed\n");
            return 1;
        }
        snprintf(ids[i], sizeof ids[i], "job-%d", i);
        jobs[i].id = ids[i];
        jobs[i].file = bufs[i];
        jobs[i].len = (size_t)need;
    }
    /* one JobsReply = one call; outs[i] answers jobs[i] */
    if (bt_run_batch(e, (size_t)n, jobs, outs) != 0) {
        fprintf(stderr, "bt_run_batch: %s\n", bt_last_error());
        rc = 1;
    } else {
        for (i = 0; i < n; ++i) {
            printf("== job %d status %d len %zu\n", i, (int)outs[i].status, outs[i].len);
            fwrite(outs[i].data, 1, outs[i].len, stdout);
        }
    }
    bt_job_out_free(outs, (size_t)n);
    bt_engine_destroy(e);
    for (i = 0; i < n; ++i) free(bufs[i]);
    free(bufs);
    free(ids);
    free(jobs);
    free(outs);
    return rc;
}

int main(int argc, char** argv) {
    if (argc >= 2 && strcmp(argv[1], "layout") == 0) return layout();
    if (argc >= 5 && strcmp(argv[1], "run") == 0)
        return run(strtoull(argv[2], NULL, 0), atoi(argv[3]), atoi(argv[4]));
    fprintf(stderr, "usage: abi_host layout | run SEED N BARS\n");
    return 2;
}
