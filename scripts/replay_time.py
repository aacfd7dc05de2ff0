"""Time Engine.replay of a sweep's top-100 against the only route to the same trade lists without
it: one one-parameter parity engine per lane (create it, load that one symbol, run, read trades).

Two datasets: a config-2 shard (5,000 symbols x 2,520 daily bars, config2_grid) and a
config-5-shaped load (64 symbols x 491,400 1-min bars, config5_grid). Each replay variant (trades
only, trades + curves) is called once to warm up and then timed three times with host clocks
around the synchronous call; the median is reported. The parity route is timed once over the same
100 lanes (it has nothing to warm up: every lane builds a new engine), and its trade lists are
compared with the replay's.

    python scripts/replay_time.py [--out profiles/replay/replay_time.json]
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

TRADE_CAP = 4096
K = 100
SYM_BEGIN = 1000
CASES = {
    "config2_shard": (D.config2_grid, 5000, 2520, D.BT_DAILY),
    "config5_shape": (D.config5_grid, 64, 491_400, D.BT_MINUTE),
}


def timed(fn, repeats=3):
    fn()  # warm-up
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), [round(t * 1e3, 3) for t in ts], out


def parity_route(grid, e, top, bars):
    """The parent commit's route, per lane: a one-parameter parity engine on that one symbol."""
    out = []
    t0 = time.perf_counter()
    for rec in top:
        kw = grid.param(int(rec["param"]))
        one = D.Grid.sma([kw["f"]], [kw["s"]], annualization=grid.annualization)
        close = e.close_column(int(rec["sym"]) - SYM_BEGIN, bars)
        with D.Engine(one, parity=True, trade_cap=TRADE_CAP) as pe:
            pe.load_ohlc([close], sym_ids=[int(rec["sym"])])
            pe.run()
            out.append((pe.summaries()[0, 0].copy(), pe.trades()[0, 0].copy()))
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {}
    for name, (mk, n_sym, bars, freq) in CASES.items():
        grid = mk()
        with D.Engine(grid, topk=K) as e:
            e.load_synthetic(0xD1CE, SYM_BEGIN, n_sym, bars, freq)
            e.run()
            top = e.read_topk()
            assert len(top) == K
            t_tr, s_tr, rp = timed(lambda: e.replay(top, trade_cap=TRADE_CAP))
            t_cv, s_cv, rc = timed(lambda: e.replay(top, trade_cap=TRADE_CAP, curves=True))
            t_par, par = parity_route(grid, e, top, bars)
        for i, (s, tr) in enumerate(par):
            assert s.tobytes() == rp.summaries[i].tobytes() == rc.summaries[i].tobytes(), (name, i)
            m = min(int(s["n_trades"]), TRADE_CAP)  # the parity rows are undefined past the trades
            for f in ("entry_bar", "exit_bar", "side", "entry_px", "exit_px"):
                assert np.array_equal(tr[f][:m], rp.trades[i][f][:m]), (name, i, f)
                assert np.array_equal(tr[f][:m], rc.trades[i][f][:m]), (name, i, f)
        res[name] = {
            "symbols": n_sym, "bars": bars, "params": grid.n_params, "lanes": K, "trade_cap": TRADE_CAP,
            "replay_trades_ms": round(t_tr * 1e3, 3),
            "replay_trades_curves_ms": round(t_cv * 1e3, 3),
            "samples_ms": {"trades": s_tr, "trades_curves": s_cv},
            "curve_bytes": int(rc.equity.nbytes + rc.pos.nbytes),
            "parity_engines_ms": round(t_par * 1e3, 3),
        }
        print(json.dumps({name: res[name]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
