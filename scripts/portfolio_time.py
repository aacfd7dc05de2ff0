"""Time Engine.portfolio against the only other route to the same rows: the per-bar curves of every
entry through Engine.replay(lanes, curves=True), 4,096 lanes per call, and a numpy column sum on
the host.

Three shapes: the per-symbol best lane of a config-2 shard (5,000 entries x 2,520 daily bars), the
walk-forward picks of the same shard (10 folds, train 3: 35,000 windowed entries) and a
config-5-shaped load (64 entries x 491,400 1-min bars, config5_grid). Each route is called once
to warm up and then timed three times with host clocks around the synchronous calls; the median
is reported, and the two routes' rows are compared. On the config-2 best lanes the replica count
is swept (R = 1, 4, 16, 64). `finish_only_ms` is a call without entries at the same T: the
accumulators zeroed, pf_finish_kernel and the copy back, no walk; the kernel's own time comes from
a kernel trace of this script (profiles/portfolio/README.md).

    python scripts/portfolio_time.py [--out profiles/portfolio/portfolio_time.json] [--case NAME]
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
CASES = ("config2_best", "config2_walk_forward", "config5_shape")


def timed(fn, repeats=3):
    fn()  # warm-up
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), [round(t * 1e3, 3) for t in ts], out


def replay_route(e, lanes, T):
    """(pnl, n_long, n_short) of PF_LANE_DTYPE entries from replayed curves, 4,096 entries a call."""
    pnl, nl, ns = np.zeros(T, np.int64), np.zeros(T, np.int32), np.zeros(T, np.int32)
    t = np.arange(T)
    for i in range(0, len(lanes), D.REPLAY_MAX):
        part = lanes[i:i + D.REPLAY_MAX]
        rp = e.replay(part, curves=True)
        d = np.diff(rp.equity, axis=1, prepend=0)
        pos = rp.pos
        to = np.minimum(part["to_bar"], rp.n_bars)
        if (part["from_bar"] > 0).any() or (to < T).any():   # entries over all T bars need no mask
            inside = (t >= part["from_bar"][:, None]) & (t < to[:, None])
            d, pos = np.where(inside, d, 0), np.where(inside, pos, 0)
        pnl += d.sum(axis=0)
        nl += (pos > 0).sum(axis=0, dtype=np.int32)
        ns += (pos < 0).sum(axis=0, dtype=np.int32)
    return pnl, nl, ns


def measure(e, lanes, T, sweep=False):
    t_pf, s_pf, pf = timed(lambda: e.portfolio(lanes, n_bars=T))
    t_rp, s_rp, (pnl, nl, ns) = timed(lambda: replay_route(e, lanes, T))
    assert np.array_equal(pf.pnl, pnl) and np.array_equal(pf.n_long, nl) and np.array_equal(pf.n_short, ns)
    assert np.array_equal(pf.equity, np.cumsum(pnl)) and int(pf.summary["pnl"]) == int(pnl.sum())
    t_fin, s_fin, _ = timed(lambda: e.portfolio(lanes[:0], n_bars=T))
    out = {
        "entries": len(lanes), "bars": T, "window_bars": int((np.minimum(lanes["to_bar"], T) - lanes["from_bar"]).clip(0).sum()),
        "portfolio_ms": round(t_pf * 1e3, 3), "replay_route_ms": round(t_rp * 1e3, 3),
        "finish_only_ms": round(t_fin * 1e3, 3),
        "samples_ms": {"portfolio": s_pf, "replay_route": s_rp, "finish_only": s_fin},
        "curve_bytes_replay_route": len(lanes) * T * 9, "result_bytes": T * 24 + 80,
        "summary": {k: (float if k == "sharpe" else int)(pf.summary[k]) for k in pf.summary.dtype.names},
    }
    if sweep:
        out["replica_sweep_ms"] = {}
        for r in (1, 4, 16, 64):
            e.set_portfolio_replicas(r)
            t, s, got = timed(lambda: e.portfolio(lanes, n_bars=T))
            assert got.pnl.tobytes() == pf.pnl.tobytes() and got.summary.tobytes() == pf.summary.tobytes()
            out["replica_sweep_ms"][str(r)] = {"median": round(t * 1e3, 3), "samples": s}
        e.set_portfolio_replicas(0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", choices=CASES, default=None)
    args = ap.parse_args()
    want = lambda name: args.case in (None, name)
    res = {}

    def report(name, r):
        res[name] = r
        print(json.dumps({name: r}), flush=True)

    if want("config2_best") or want("config2_walk_forward"):
        grid, n_sym, bars = D.config2_grid(), 5000, 2520
        with D.Engine(grid) as e:
            e.load_synthetic(0xD1CE, SYM_BEGIN, n_sym, bars, D.BT_DAILY)
            if want("config2_best"):
                e.run()
                report("config2_best", measure(e, D.as_pf_lanes(e.surface().best), bars, sweep=True))
            if want("config2_walk_forward"):
                wf = e.walk_forward([bars * k // FOLDS for k in range(FOLDS + 1)], train=TRAIN)
                report("config2_walk_forward", measure(e, D.walk_forward_lanes(wf), bars))
    if want("config5_shape"):
        grid, n_sym, bars = D.config5_grid(), 64, 491_400
        with D.Engine(grid) as e:
            e.load_synthetic(0xD1CE, SYM_BEGIN, n_sym, bars, D.BT_MINUTE)
            lanes = D.as_pf_lanes([(SYM_BEGIN + s, (s * 37) % grid.n_params) for s in range(n_sym)])
            report("config5_shape", measure(e, lanes, bars))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
