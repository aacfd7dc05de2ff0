"""Time Engine.costs on the config-2 shard (5,000 symbols x 2,520 daily bars, 400 params) at C = 8
levels against the only other route to the same figures: Engine.replay with complete trade lists
and equity curves, up to 4,096 lanes per call, and costs_host lane by lane on the host.

Host clocks around the synchronous call, one warm-up, the median of three:

  A  costs(levels, per_lane=False, params=True): the aggregates alone, nothing S x P leaves the device;
  B  costs(levels): every (lane, level) record copied to the host;
  D  replay(lanes, trade_cap, curves=True) of the first 4,096 lanes (row-major over symbols and
     params) plus costs_host on each, timed once after a warm-up and SCALED to S*P lanes:
     `replay_route_scaled_ms` is that figure times S*P / lanes, not a measurement of the whole.

The records of route D's lanes are compared with the device's, byte for byte. `--kernels` runs A
three times and nothing else, for a kernel trace in a run of its own.

    python scripts/costs_time.py [--out profiles/costs/costs_time.json] [--levels 8] [--kernels]
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
N_SYM, BARS = 5000, 2520
# free, one tick and five ticks a side, 1 / 2 / 5 / 10 basis points, and a mixed level
LADDER = [(0, 0), (1, 0), (5, 0), (0, 1), (0, 2), (0, 5), (0, 10), (2, 3), (10, 5), (0, 20), (20, 0), (3, 7),
          (50, 0), (0, 50), (7, 13), (100, 100)]


def timed(fn, repeats=3):
    fn()  # warm-up
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), [round(t * 1e3, 3) for t in ts], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--levels", type=int, default=8)
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    levels = LADDER[:args.levels]
    C = len(levels)
    grid = D.config2_grid()
    P = grid.n_params
    with D.Engine(grid) as e:
        e.load_synthetic(0xD1CE, SYM_BEGIN, N_SYM, BARS, D.BT_DAILY)
        if args.kernels:
            for _ in range(3):
                e.costs(levels, per_lane=False, params=True)
            print(json.dumps({"config2_shard": "kernels"}), flush=True)
            return
        t_a, s_a, agg = timed(lambda: e.costs(levels, per_lane=False, params=True))
        t_b, s_b, full = timed(lambda: e.costs(levels))
        assert np.array_equal(D.costs_agg_host(full.lanes), agg.params)
        t_ts, s_ts, _ = timed(lambda: e.trade_stats(per_lane=False, params=True))
        n = min(D.REPLAY_MAX, N_SYM * P)
        lanes = [(SYM_BEGIN + i // P, i % P) for i in range(n)]
        cap = max(int(full.lanes.reshape(-1, C)[:n, 0]["n_trades"].max()), 1)

        def route():
            rp = e.replay(lanes, trade_cap=cap, curves=True)
            out = np.zeros((n, C), D.COST_DTYPE)
            for i in range(n):
                out[i] = D.costs_host(rp.trades[i, :rp.summaries["n_trades"][i]], rp.equity[i, :rp.n_bars[i]], levels)
            return out
        route()  # warm-up
        t0 = time.perf_counter()
        ref = route()
        t_d = time.perf_counter() - t0
    assert ref.tobytes() == np.ascontiguousarray(full.lanes.reshape(-1, C)[:n]).tobytes(), "route D differs"
    scale = N_SYM * P / n
    free = agg.params[:, 0]
    res = {"config2_shard": {
        "symbols": N_SYM, "bars": BARS, "params": P, "lanes": N_SYM * P, "levels": [list(x) for x in levels],
        "A_agg_only_ms": round(t_a * 1e3, 3), "B_all_records_ms": round(t_b * 1e3, 3),
        "trade_stats_agg_only_ms": round(t_ts * 1e3, 3),
        "samples_ms": {"A": s_a, "B": s_b, "trade_stats": s_ts},
        "record_bytes_all_lanes": N_SYM * P * C * D.COST_DTYPE.itemsize, "agg_bytes": P * C * D.COST_AGG_DTYPE.itemsize,
        "replay_route_lanes": n, "replay_route_trade_cap": cap, "replay_route_ms": round(t_d * 1e3, 1),
        "scale": round(scale, 3), "replay_route_scaled_ms": round(t_d * 1e3 * scale, 1),
        "lanes_checked_against_the_route": n,
        "trades": int(free["trades"].sum()),
        "survivors_per_level": [round(float(x), 4) for x in agg.survivors().mean(axis=0)],
        "params_with_positive_total_per_level": [int((agg.params["pnl"][:, j] > 0).sum()) for j in range(C)],
    }}
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
