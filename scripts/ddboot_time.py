"""Time Engine.drawdown_risk against the only other route to the same figures: Engine.replay with
equity curves and bt_drawdown_boot_host (drawdown_risk_host), which draws the bars one by one.

Host clocks around the synchronous call, one warm-up, medians:

  config-2 shard (5,000 symbols x 2,520 daily bars, 400 params), B = 1,000, L = 10, two levels:
    L / A  all-lanes mode under set_ddboot_row(1) (the row in LDS: 97,864 bytes a workgroup with
           scratch and values, one workgroup a CU) and set_ddboot_row(2) (rows in the arena),
           ALTERNATED call by call for `--rounds` rounds: the planner's row rule is judged on these
           two columns and on their run-to-run spread;
    P      the planner's own choice (set_ddboot_row(0)), once more;
    B      the 5,000 best-per-symbol lanes (surface().best) in list mode, in both homes;
    H      replay(lanes, curves=True) of the first `--host-lanes` lanes plus drawdown_risk_host on
           them, timed once after a warm-up and SCALED to S * P lanes: `host_route_scaled_ms` is that
           figure times S * P / lanes, not a measurement of the whole.

The device's figures of the host route's lanes are compared with the host's, byte for byte.

    python scripts/ddboot_time.py [--out profiles/ddboot/ddboot_time.json] [--rounds 3] [--host-lanes 64]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dbx_amd as D  # noqa: E402

SYM_BEGIN = 1000
N_SYM, BARS = 5000, 2520
B, L, SEED = 1000, 10, 0xDD
LEVELS = (0.5, 0.95)


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def stats(ts):
    return {"median_ms": round(statistics.median(ts) * 1e3, 3), "min_ms": round(min(ts) * 1e3, 3),
            "max_ms": round(max(ts) * 1e3, 3), "samples_ms": [round(t * 1e3, 3) for t in ts]}


def same(a, b):
    return a.lanes.tobytes() == b.lanes.tobytes() and a.quantiles.tobytes() == b.quantiles.tobytes()


def alternate(e, call, rounds):
    """{row: [seconds]} of `call` under the two forced homes, alternated, after a warm-up of each."""
    t, first = {1: [], 2: []}, None
    for row in (1, 2):
        e.set_ddboot_row(row)
        call()
    for _ in range(rounds):
        for row in (1, 2):
            e.set_ddboot_row(row)
            dt, out = clock(call)
            assert e.last_ddboot_row() == row
            t[row].append(dt)
            first = first or out
            assert same(out, first), "the two homes return the same bytes"
    e.set_ddboot_row(0)
    return t, first


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-lanes", type=int, default=64)
    ap.add_argument("--symbols", type=int, default=N_SYM)
    args = ap.parse_args()
    grid = D.config2_grid()
    P, S = grid.n_params, args.symbols
    res = {}
    with D.Engine(grid) as e:
        e.load_synthetic(0xD1CE, SYM_BEGIN, S, BARS, D.BT_DAILY)
        t, all_lanes = alternate(e, lambda: e.drawdown_risk(None, B, L, SEED, None, LEVELS), args.rounds)
        print(json.dumps({"lds_row": stats(t[1]), "arena_row": stats(t[2])}), flush=True)
        t_p, own = clock(lambda: e.drawdown_risk(None, B, L, SEED, None, LEVELS))
        home = e.last_ddboot_row()
        assert same(own, all_lanes)
        e.run()
        best = e.surface().best
        t_b, best_lanes = alternate(e, lambda: e.drawdown_risk(best, B, L, SEED, None, LEVELS), args.rounds)
        n = min(args.host_lanes, S * P)
        lanes = [(SYM_BEGIN + i // P, i % P) for i in range(n)]

        def host_route(req):
            rp = e.replay(req, curves=True)
            return D.drawdown_risk_host(rp.equity, rp.n_bars, B, L, SEED, (0, BARS), LEVELS)

        host_route(lanes[:2])      # warm-up
        t_h, ref = clock(lambda: host_route(lanes))
        assert ref.lanes.tobytes() == all_lanes.lanes.reshape(-1)[:n].tobytes()
        assert ref.quantiles.tobytes() == all_lanes.quantiles.reshape(-1, len(LEVELS))[:n].tobytes()
        scale = S * P / n
        res["config2_shard"] = {
            "symbols": S, "bars": BARS, "params": P, "lanes": S * P, "resamples": B, "block": L, "levels": list(LEVELS),
            "lds_row": stats(t[1]), "arena_row": stats(t[2]), "planner_home": home, "planner_home_ms": round(t_p * 1e3, 3),
            "best_per_symbol_lanes": len(best), "best_lds_row": stats(t_b[1]), "best_arena_row": stats(t_b[2]),
            "host_route_lanes": n, "host_route_ms": round(t_h * 1e3, 1), "scale": round(scale, 3),
            "host_route_scaled_ms": round(t_h * 1e3 * scale, 1), "lanes_checked_against_the_route": n,
        }
        print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
