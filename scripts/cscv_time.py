"""Time Engine.cscv against the only other route to the same figures: Engine.walk_forward's fold
records of some rows and bt_cscv_host on them.

  sweep10, sweep16   the config-2 shard (5,000 symbols x 2,520 daily bars, 400 params), K = 10 and
          K = 16 equal folds, one group per symbol, groups and histograms (no picks). Host clocks
          around the synchronous call, one warm-up, the median of three:
            A  cscv(bounds): walk, pack and combinations;
            W  walk_forward(bounds): the walk and one selection per step, the walk's share;
            D  walk_forward(folds=True) of the first symbols plus cscv_host, timed once and SCALED
               to the shard's symbols: `host_route_scaled_ms` is that figure times S / symbols, not a
               measurement of the whole. Its group records are compared with the device's.
          `pair_cells` is rows x pairs x P, the unit of bt_set_cscv_work; `cells_per_s` divides it
          by A - W, so it charges the pack and the copies to the combination kernel.
  long    64 lanes on the config-5 axes x 491,400 1-min bars, K = 16: one group, the walk dominates.

`--kernels` runs A three times per case and nothing else: under a kernel trace (`rocprofv3
--kernel-trace --stats`, a run of its own) or a counter run (`--pmc`, another run of its own) that
gives the figures of cscv_kernel. `--work CELLS` sets bt_set_cscv_work.

    python scripts/cscv_time.py [--out profiles/cscv/cscv_time.json] [--case NAME] [--no-host] [--kernels] [--work CELLS]
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
HOST_SYMBOLS = 2


def timed(fn, repeats=3):
    fn()  # warm-up
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), [round(t * 1e3, 3) for t in ts], out


def case(grid, n_sym, bars, freq, K, kernels, host, work):
    P = grid.n_params
    bounds = [bars * k // K for k in range(K + 1)]
    C = len(D.cscv_combos(K))
    with D.Engine(grid) as e:
        e.load_synthetic(0xD1CE, SYM_BEGIN, n_sym, bars, freq)
        e.set_cscv_work(work)
        if kernels:
            for _ in range(3):
                e.cscv(bounds, hist=True)
            return "kernels"
        t_a, s_a, a = timed(lambda: e.cscv(bounds, hist=True))
        t_w, s_w, _ = timed(lambda: e.walk_forward(bounds))
        t_d = None
        n_host = min(HOST_SYMBOLS, n_sym)
        if host:
            with D.Engine(grid) as h:
                h.load_synthetic(0xD1CE, SYM_BEGIN, n_host, bars, freq)
                t0 = time.perf_counter()
                wf = h.walk_forward(bounds, folds=True)
                ref = D.cscv_host(wf.folds, range(SYM_BEGIN, SYM_BEGIN + n_host), grid.annualization, hist=True)
                t_d = time.perf_counter() - t0
            assert ref.groups.tobytes() == a.groups[:n_host].tobytes(), "the host route disagrees with the device"
            assert ref.hist.tobytes() == a.hist[:n_host].tobytes()
    cells = n_sym * (C // 2) * P
    pbo = a.pbo()
    return {
        "symbols": n_sym, "bars": bars, "params": P, "folds": K, "combinations": C, "pair_cells": cells,
        "lane_combinations": 2 * cells, "A_cscv_ms": round(t_a * 1e3, 3), "W_walk_forward_ms": round(t_w * 1e3, 3),
        "samples_ms": {"A": s_a, "W": s_w},
        "cells_per_s": round(cells / max(t_a - t_w, 1e-9), 1),
        "host_route_symbols": n_host if host else 0, "host_route_ms": round(t_d * 1e3, 1) if host else None,
        "scale": n_sym / n_host, "host_route_scaled_ms": round(t_d * 1e3 * n_sym / n_host, 1) if host else None,
        "pbo_median": float(np.median(pbo)), "pbo_above_0.5": int((pbo > 0.5).sum()),
        "prob_loss_median": float(np.median(a.prob_loss())), "dead": int(a.groups["n_dead"].sum()),
    }


def long_grid():
    return D.Grid.sma(range(5, 161, 20), range(200, 6401, 800), annualization=98280)   # 64 lanes of config 5's axes


CASES = {
    "sweep10": lambda k, h, w: case(D.config2_grid(), 5000, 2520, D.BT_DAILY, 10, k, h, w),
    "sweep16": lambda k, h, w: case(D.config2_grid(), 5000, 2520, D.BT_DAILY, 16, k, h, w),
    "long": lambda k, h, w: case(long_grid(), 1, 491_400, D.BT_MINUTE, 16, k, h, w),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", choices=list(CASES), default=None)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--work", type=int, default=0)
    args = ap.parse_args()
    res = {}
    for name, fn in CASES.items():
        if args.case and name != args.case:
            continue
        res[name] = fn(args.kernels, not args.no_host, args.work)
        print(json.dumps({name: res[name]}), flush=True)
    if args.out and res and not args.kernels:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
