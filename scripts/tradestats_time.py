"""Time Engine.trade_stats against the only other route to the same figures: Engine.replay with
complete trade lists and equity curves, up to 4,096 lanes per call, reduced to the statistics with
numpy on the host.

Three shards: config 2 (5,000 symbols x 2,520 daily bars, 400 params), and the 500-symbol shards of
config 3 (98,280 1-min bars, 64 params) and config 4 (98,280 1-min bars, 256 params). Per shard,
host clocks around the synchronous call, one warm-up, the median of three:

  A  trade_stats(per_lane=False, params=True): the aggregates alone, nothing S x P leaves the device;
  B  trade_stats(): every lane's record copied to the host;
  D  replay(lanes, trade_cap, curves=True) of the first lanes (row-major over symbols and params;
     4,096 of them, fewer when their curves would pass 1 GB) plus the numpy statistics, timed once
     after a warm-up and SCALED to S*P lanes: `replay_route_scaled_ms` is that figure times
     S*P / lanes, not a measurement of the whole.

The records of route D's lanes are compared with the device's. `--kernels` runs A and the
walk-forward of the single fold [0, B) three times each and nothing else: under a kernel trace
(`rocprofv3 --kernel-trace --stats`, a run of its own) that gives the times of tstats_walk_kernel
and of wf_walk_kernel (C) on the same shard.

    python scripts/tradestats_time.py [--out profiles/tradestats/tradestats_time.json] [--case NAME] [--kernels]
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
CASES = {
    "config2_shard": (D.config2_grid, 5000, 2520, D.BT_DAILY),
    "config3_shard": (D.config3_grid, 500, 98_280, D.BT_MINUTE),
    "config4_shard": (D.config4_grid, 500, 98_280, D.BT_MINUTE),
}
CURVE_BYTES = 1 << 30
CHECKED = ("n_trades", "n_win", "n_loss", "max_win_streak", "max_loss_streak", "hold_sum", "hold_max", "gross_win",
           "gross_loss", "max_win", "max_loss", "mdd", "mdd_bar", "peak_bar", "underwater_bars", "max_underwater")


def timed(fn, repeats=3):
    fn()  # warm-up
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), [round(t * 1e3, 3) for t in ts], out


def longest_run(flags):
    """Longest run of True in a 1-D bool array."""
    if not flags.any():
        return 0
    edges = np.diff(np.concatenate(([0], flags.astype(np.int8), [0])))
    return int((np.nonzero(edges < 0)[0] - np.nonzero(edges > 0)[0]).max())


def numpy_stats(trades, n_trades, equity, n_bars):
    """The checked fields of every lane from its trade list and equity curve, in numpy."""
    out = np.zeros(len(trades), [(f, np.int64) for f in CHECKED])
    for i in range(len(trades)):
        t = trades[i, :n_trades[i]]
        pnl = t["side"].astype(np.int64) * (t["exit_px"] - t["entry_px"])
        hold = (t["exit_bar"] - t["entry_bar"]).astype(np.int64)
        win, loss = pnl > 0, pnl < 0
        eq = equity[i, :n_bars[i]]
        peak = np.maximum.accumulate(np.maximum(eq, 0))
        dd = peak - eq
        at = int(dd.argmax())
        r = out[i]
        r["n_trades"], r["n_win"], r["n_loss"] = len(t), win.sum(), loss.sum()
        r["max_win_streak"], r["max_loss_streak"] = longest_run(win), longest_run(loss)
        r["hold_sum"], r["hold_max"] = hold.sum(), hold.max(initial=0)
        r["gross_win"], r["gross_loss"] = pnl[win].sum(), -pnl[loss].sum()
        r["max_win"], r["max_loss"] = pnl[win].max(initial=0), (-pnl[loss]).max(initial=0)
        r["mdd"] = dd[at]
        r["mdd_bar"] = at if dd[at] > 0 else -1
        r["peak_bar"] = int(np.argmax(eq[:at + 1] == peak[at])) if dd[at] > 0 else -1
        r["underwater_bars"], r["max_underwater"] = (dd > 0).sum(), longest_run(dd > 0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", choices=list(CASES), default=None)
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    res = {}
    for name, (mk, n_sym, bars, freq) in CASES.items():
        if args.case and name != args.case:
            continue
        grid = mk()
        P = grid.n_params
        with D.Engine(grid) as e:
            e.load_synthetic(0xD1CE, SYM_BEGIN, n_sym, bars, freq)
            if args.kernels:
                for _ in range(3):
                    e.trade_stats(per_lane=False, params=True)
                    e.walk_forward([0, bars, bars + 1], train=1)   # fold 0 = [0, B), fold 1 empty
                print(json.dumps({name: "kernels"}), flush=True)
                continue
            t_a, s_a, agg = timed(lambda: e.trade_stats(per_lane=False, params=True))
            t_b, s_b, full = timed(lambda: e.trade_stats())
            assert np.array_equal(D.trade_stats_agg_host(full.lanes), agg.params), name
            n = min(D.REPLAY_MAX, n_sym * P, max(CURVE_BYTES // (bars * 9), 1))
            lanes = [(SYM_BEGIN + i // P, i % P) for i in range(n)]
            cap = max(int(full.lanes.reshape(-1)[:n]["n_trades"].max()), 1)

            def route():
                rp = e.replay(lanes, trade_cap=cap, curves=True)
                return numpy_stats(rp.trades, rp.summaries["n_trades"], rp.equity, rp.n_bars)
            route()  # warm-up
            t0 = time.perf_counter()
            ref = route()
            t_d = time.perf_counter() - t0
        dev = full.lanes.reshape(-1)[:n]
        for f in CHECKED:
            assert np.array_equal(ref[f], dev[f].astype(np.int64)), (name, f)
        scale = n_sym * P / n
        res[name] = {
            "symbols": n_sym, "bars": bars, "params": P, "lanes": n_sym * P,
            "A_agg_only_ms": round(t_a * 1e3, 3), "B_all_records_ms": round(t_b * 1e3, 3),
            "samples_ms": {"A": s_a, "B": s_b},
            "record_bytes_all_lanes": n_sym * P * D.TSTATS_DTYPE.itemsize,
            "agg_bytes": P * D.TSTATS_AGG_DTYPE.itemsize,
            "replay_route_lanes": n, "replay_route_trade_cap": cap,
            "replay_route_ms": round(t_d * 1e3, 1), "scale": round(scale, 3),
            "replay_route_scaled_ms": round(t_d * 1e3 * scale, 1),
            "lanes_checked_against_the_route": n,
            "trades": int(agg.params["n_trades"].sum()),
            "win_rate": float(agg.params["n_win"].sum() / max(int(agg.params["n_trades"].sum()), 1)),
            "best_profit_factor": float(agg.profit_factor().max()),
            "longest_loss_streak": int(agg.params["max_loss_streak"].max()),
            "longest_underwater_bars": int(agg.params["max_underwater"].max()),
        }
        print(json.dumps({name: res[name]}), flush=True)
    if args.out and res:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
