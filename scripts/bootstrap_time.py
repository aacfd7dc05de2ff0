"""Time Engine.reality_check against the only other route to the same figures: Engine.replay with
equity curves of every lane of a symbol, and the block bootstrap on the host (reality_check_host).

  sweep   the config-2 shard (5,000 symbols x 2,520 daily bars, 400 params), all-lanes mode, one
          group per symbol, B = 1000 resamples in blocks of L = 10. Host clocks around the synchronous
          call, one warm-up, the median of three:
            A  reality_check(): the 5,000 group records alone;
            B  reality_check(per_lane=True, vmax=True): every lane record and V* too;
            W  reality_check(resamples=1): the walk with one resample, the walk's share;
            Wt the same over the window [3/4 bars, bars): the whole walk, a quarter of the prefix row
               (a quarter of the LDS per workgroup);
            D  replay(curves=True) of the first symbols' lanes plus reality_check_host, timed once
               and SCALED to the shard's symbols: `host_route_scaled_ms` is that figure times
               S / symbols, not a measurement of the whole. Its group records are compared with the
               device's.
  arena   64 lanes x 491,400 1-min bars (one symbol of the config-3 grid), B = 1000, L = 100: the
          prefix rows live in device memory. `gathered_bytes` is n * B * K * 16.

`--no-host` leaves D out (for A/B builds of the library, BT_LIB). `--kernels` runs A and W and
trade_stats(per_lane=False, params=True) three times each and nothing else: under a kernel trace (`rocprofv3 --kernel-trace --stats`, a run of its own) that gives the
times of boot_kernel at B = 1000 and B = 1 and of tstats_walk_kernel over the same lanes.

    python scripts/bootstrap_time.py [--out profiles/bootstrap/bootstrap_time.json] [--case NAME] [--no-host] [--kernels]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dbx_amd as D  # noqa: E402

SYM_BEGIN = 1000
B, SEED = 1000, 0xB007
HOST_SYMBOLS = 2


def timed(fn, repeats=3):
    fn()  # warm-up
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), [round(t * 1e3, 3) for t in ts], out


def sweep(kernels, host=True):
    grid, n_sym, bars, L = D.config2_grid(), 5000, 2520, 10
    P = grid.n_params
    K = -(-bars // L)
    with D.Engine(grid) as e:
        e.load_synthetic(0xD1CE, SYM_BEGIN, n_sym, bars, D.BT_DAILY)
        if kernels:
            for _ in range(3):
                e.reality_check(resamples=B, block=L, seed=SEED)
                e.reality_check(resamples=1, block=L, seed=SEED)
                e.trade_stats(per_lane=False, params=True)
            return "kernels"
        t_a, s_a, a = timed(lambda: e.reality_check(resamples=B, block=L, seed=SEED))
        t_b, s_b, b = timed(lambda: e.reality_check(resamples=B, block=L, seed=SEED, per_lane=True, vmax=True))
        t_w, s_w, _ = timed(lambda: e.reality_check(resamples=1, block=L, seed=SEED))
        t_t, s_t, _ = timed(lambda: e.reality_check(resamples=1, block=L, seed=SEED, window=(bars * 3 // 4, bars)))
        assert a.groups.tobytes() == b.groups.tobytes()
        lanes = [(SYM_BEGIN + i // P, i % P) for i in range(HOST_SYMBOLS * P)]

        def route():
            rp = e.replay(lanes, curves=True)
            return D.reality_check_host(rp.equity, rp.n_bars, groups=[P] * HOST_SYMBOLS, resamples=B, block=L, seed=SEED)
        t_d = None
        if host:
            t0 = time.perf_counter()
            ref = route()
            t_d = time.perf_counter() - t0
            assert ref.groups.tobytes() == a.groups[:HOST_SYMBOLS].tobytes(), "the host route disagrees with the device"
    p = a.p_value()
    return {
        "symbols": n_sym, "bars": bars, "params": P, "lanes": n_sym * P, "resamples": B, "block": L, "blocks": K,
        "A_groups_only_ms": round(t_a * 1e3, 3), "B_lanes_and_vmax_ms": round(t_b * 1e3, 3),
        "W_one_resample_ms": round(t_w * 1e3, 3), "Wt_one_resample_last_quarter_ms": round(t_t * 1e3, 3),
        "samples_ms": {"A": s_a, "B": s_b, "W": s_w, "Wt": s_t},
        "lds_reads_per_lane": -(-B // 64) * K * 2,
        "host_route_symbols": HOST_SYMBOLS if host else 0, "host_route_ms": round(t_d * 1e3, 1) if host else None,
        "scale": n_sym / HOST_SYMBOLS, "host_route_scaled_ms": round(t_d * 1e3 * n_sym / HOST_SYMBOLS, 1) if host else None,
        "groups_checked_against_the_route": HOST_SYMBOLS if host else 0,
        "p_below_0.05": int((p < 0.05).sum()), "p_below_0.01": int((p < 0.01).sum()), "p_median": float(np.median(p)),
    }


def arena(kernels, host=True):
    grid, bars, L = D.config3_grid(), 491_400, 100
    P = grid.n_params
    K = -(-bars // L)
    with D.Engine(grid) as e:
        e.load_synthetic(0xD1CE, SYM_BEGIN, 1, bars, D.BT_MINUTE)
        if kernels:
            for _ in range(3):
                e.reality_check(resamples=B, block=L, seed=SEED)
            return "kernels"
        t_a, s_a, a = timed(lambda: e.reality_check(resamples=B, block=L, seed=SEED))
        t_w, s_w, _ = timed(lambda: e.reality_check(resamples=1, block=L, seed=SEED))
    return {"lanes": P, "bars": bars, "resamples": B, "block": L, "blocks": K,
            "A_groups_only_ms": round(t_a * 1e3, 3), "W_one_resample_ms": round(t_w * 1e3, 3),
            "samples_ms": {"A": s_a, "W": s_w}, "gathered_bytes": P * B * K * 16,
            "p_value": float(a.p_value()[0])}


CASES = {"sweep": sweep, "arena": arena}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", choices=list(CASES), default=None)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    res = {}
    for name, fn in CASES.items():
        if args.case and name != args.case:
            continue
        res[name] = fn(args.kernels, not args.no_host)
        print(json.dumps({name: res[name]}), flush=True)
    if args.out and res and not args.kernels:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
