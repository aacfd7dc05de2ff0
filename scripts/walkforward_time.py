"""Time Engine.walk_forward against the only other route to the same numbers: the per-bar curves
of every lane through Engine.replay(lanes, curves=True), 4,096 lanes per call, reduced to fold
records with numpy on the host.

Two datasets: a config-2 shard (5,000 symbols x 2,520 daily bars, config2_grid, 400 params) and a
config-3-shaped load (64 symbols x 49,140 1-min bars, config3_grid, 64 params), each with 10 equal
folds and train=3. walk_forward (steps and totals) is called once to warm up and then timed three
times with host clocks around the synchronous call; the median is reported. The replay route is
timed the same way on the first 4,096 lanes (row-major over symbols and params) and SCALED to S*P
lanes: `replay_route_scaled_ms` is that figure times S*P / 4,096, not a measurement of the whole.
Its fold reduction computes pnl, mdd, exposure and float64 return sums per fold (no int128), which
favours it.

    python scripts/walkforward_time.py [--out profiles/walkforward/walkforward_time.json] [--case NAME]
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
FOLDS, TRAIN = 10, 3
CASES = {
    "config2_shard": (D.config2_grid, 5000, 2520, D.BT_DAILY),
    "config3_shape": (D.config3_grid, 64, 49_140, D.BT_MINUTE),
}


def timed(fn, repeats=3):
    fn()  # warm-up
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), [round(t * 1e3, 3) for t in ts], out


def fold_reduce(eq, pos, q, row, bounds):
    """Fold records of n lanes from their curves (lane i is a lane of symbol row[i], whose returns are
    q[row[i]]): (pnl, mdd, exposure, s1, s2), each [n, K]."""
    n, K = len(eq), len(bounds) - 1
    out = [np.zeros((n, K), np.int64) for _ in range(3)] + [np.zeros((n, K)) for _ in range(2)]
    for k in range(K):
        c0, c1 = bounds[k], bounds[k + 1]
        base = eq[:, c0 - 1] if c0 else np.zeros(n, np.int64)
        d = eq[:, c0:c1] - base[:, None]
        peak = np.maximum.accumulate(np.maximum(d, 0), axis=1)
        r0 = max(c0, 1)
        prev = pos[:, r0 - 1:c1 - 1].astype(np.float64)
        out[0][:, k] = eq[:, c1 - 1] - base
        out[1][:, k] = (peak - d).max(axis=1)
        out[2][:, k] = np.count_nonzero(prev, axis=1)
        qk = q[:, r0:c1][row]
        out[3][:, k] = (prev * qk).sum(axis=1)
        out[4][:, k] = (np.abs(prev) * qk ** 2).sum(axis=1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", choices=list(CASES), default=None)
    args = ap.parse_args()
    res = {}
    for name, (mk, n_sym, bars, freq) in CASES.items():
        if args.case and name != args.case:
            continue
        grid = mk()
        P = grid.n_params
        bounds = [bars * k // FOLDS for k in range(FOLDS + 1)]
        with D.Engine(grid) as e:
            e.load_synthetic(0xD1CE, SYM_BEGIN, n_sym, bars, freq)
            t_wf, s_wf, wf = timed(lambda: e.walk_forward(bounds, train=TRAIN))
            lanes = [(SYM_BEGIN + i // P, i % P) for i in range(min(D.REPLAY_MAX, n_sym * P))]
            syms = sorted({s for s, _ in lanes})
            close = np.stack([e.close_column(s - SYM_BEGIN, bars) for s in syms]).astype(np.float64)
            q = np.zeros_like(close)
            q[:, 1:] = close[:, 1:] / close[:, :-1] - 1.0
            row = np.array([syms.index(s) for s, _ in lanes])

            def route():
                rp = e.replay(lanes, curves=True)
                return rp, fold_reduce(rp.equity, rp.pos, q, row, bounds)
            t_rp, s_rp, (rp, rec) = timed(route)
        # the two routes agree where they overlap: the chosen lanes' out-of-sample pnl and drawdown
        checked = 0
        for st in wf.steps.reshape(-1):
            i = (int(st["sym"]) - SYM_BEGIN) * P + int(st["param"])
            if st["param"] >= 0 and i < len(lanes):
                assert int(rec[0][i, st["fold"]]) == int(st["oos"]["pnl"]), (name, i)
                assert int(rec[1][i, st["fold"]]) == int(st["oos"]["mdd"]), (name, i)
                assert int(rec[2][i, st["fold"]]) == int(st["oos"]["exposure"]), (name, i)
                checked += 1
        scale = n_sym * P / len(lanes)
        res[name] = {
            "symbols": n_sym, "bars": bars, "params": P, "folds": FOLDS, "train": TRAIN,
            "walk_forward_ms": round(t_wf * 1e3, 3),
            "samples_ms": {"walk_forward": s_wf, "replay_route_4096": s_rp},
            "replay_route_4096_lanes_ms": round(t_rp * 1e3, 3),
            "replay_route_lanes": len(lanes), "scale": round(scale, 3),
            "replay_route_scaled_ms": round(t_rp * 1e3 * scale, 1),
            "curve_bytes_all_lanes": int(n_sym) * P * bars * 9,
            "steps_checked_against_the_route": checked,
            "picked_steps": int((wf.steps["param"] >= 0).sum()),
            "mean_oos_sharpe": float(wf.oos_sharpe().mean()),
            "mean_train_sharpe": float(wf.train_sharpe().mean()),
        }
        print(json.dumps({name: res[name]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
