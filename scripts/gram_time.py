"""Time Engine.covariance against the only other route to a covariance of chosen lanes: their
equity curves through Engine.replay(lanes, curves=True), 4,096 lanes per call, then np.diff and a
float64 np.cov on the host. That route is not exact (it re-associates floating-point sums); the
script reports how far it lands from the exact matrix instead of asserting equality.

Three shapes: the per-symbol best lanes of a config-2 shard of 2,048 symbols (2,048 x 2,520 daily
bars), the first 256 of them, and a config-5-shaped load (64 lanes x 491,400 1-min bars,
config5_grid). Each route is called once to warm up and then timed three times with host clocks
around the synchronous calls; the median is reported. `split_sweep_ms` times forced bar-chunk
counts on the long shape. The Gram kernel's own time comes from a kernel trace of this script with
--case, in a run of its own (profiles/covariance/README.md).

    python scripts/gram_time.py [--out profiles/covariance/gram_time.json] [--case NAME]
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
CASES = ("config2_2048", "config2_256", "config5_shape")


def timed(fn, repeats=3):
    fn()  # warm-up
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), [round(t * 1e3, 3) for t in ts], out


def replay_route(e, lanes):
    """Float64 covariance (divided by T, like Covariance.cov) from replayed curves."""
    rows = []
    for i in range(0, len(lanes), D.REPLAY_MAX):
        rp = e.replay(lanes[i:i + D.REPLAY_MAX], curves=True)
        rows.append(np.diff(rp.equity, axis=1, prepend=0).astype(np.float64))
    return np.cov(np.concatenate(rows), bias=True)


def measure(e, lanes, bars, split_sweep=()):
    t_cv, s_cv, cv = timed(lambda: e.covariance(lanes))
    t_rp, s_rp, approx = timed(lambda: replay_route(e, lanes))
    exact = cv.cov()
    scale = float(np.abs(exact).max()) or 1.0
    n = len(lanes)
    nt = (n + 15) // 16
    pitch = (bars + 63) // 64 * 64
    out = {
        "lanes": n, "bars": cv.n_bars,
        "covariance_ms": round(t_cv * 1e3, 3), "replay_route_ms": round(t_rp * 1e3, 3),
        "samples_ms": {"covariance": s_cv, "replay_route": s_rp},
        "curve_bytes_replay_route": n * bars * 9, "result_bytes": n * n * 16 + n * 8,
        # what gram_mfma_kernel executes: one instruction of 16 x 16 x 4 x 2 flop per accumulator, 4 bars and tile
        "mfma_flop": nt * (nt + 1) // 2 * (pitch // 4) * 4 * 2048,
        "replay_route_max_abs_diff_over_max_cov": float(np.abs(approx - exact).max()) / scale,
        "trace_abs": float(np.trace(exact)),
    }
    if split_sweep:
        out["split_sweep_ms"] = {}
        for k in split_sweep:
            e.set_gram_split(k)
            t, s, got = timed(lambda: e.covariance(lanes))
            assert got.wide.tobytes() == cv.wide.tobytes() and got.sums.tobytes() == cv.sums.tobytes()
            out["split_sweep_ms"][str(k)] = {"median": round(t * 1e3, 3), "samples": s}
        e.set_gram_split(0)
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

    if want("config2_2048") or want("config2_256"):
        grid, n_sym, bars = D.config2_grid(), 2048, 2520
        with D.Engine(grid) as e:
            e.load_synthetic(0xD1CE, SYM_BEGIN, n_sym, bars, D.BT_DAILY)
            e.run()
            best = D.as_lanes(e.surface().best)
            if want("config2_2048"):
                report("config2_2048", measure(e, best, bars))
            if want("config2_256"):
                report("config2_256", measure(e, best[:256], bars, split_sweep=(1, 2, 5, 20)))
    if want("config5_shape"):
        grid, n_sym, bars = D.config5_grid(), 64, 491_400
        with D.Engine(grid) as e:
            e.load_synthetic(0xD1CE, SYM_BEGIN, n_sym, bars, D.BT_MINUTE)
            lanes = D.as_lanes([(SYM_BEGIN + s, (s * 37) % grid.n_params) for s in range(n_sym)])
            report("config5_shape", measure(e, lanes, bars, split_sweep=(1, 16, 1000)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
