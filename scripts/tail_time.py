"""Time Engine.tail_risk against the only other route to the same figures: Engine.replay with equity
and position curves, up to 4,096 lanes per call, and numpy on the host (np.diff, np.partition, the
power sums in Python ints).

Host clocks around the synchronous call, one warm-up, medians:

  config-2 shard (5,000 symbols x 2,520 daily bars, 400 params, Q = 3), all-lanes mode:
    L / A  set_tail_row(1) and set_tail_row(2), ALTERNATED call by call for `--rounds` rounds: the
           planner's row rule is judged on these two columns and on their run-to-run spread;
    R      the records alone (q_out = NULL through the C entry point: the walk and the sums, no
           selection), under the LDS home; L - R is the selection's share of the call;
    H      replay(lanes, curves=True) of the first `--host-lanes` lanes plus the host figures of each, timed
           once after a warm-up and SCALED to S * P lanes: `host_route_scaled_ms` is that figure
           times S * P / lanes, not a measurement of the whole;
  minute rows (8 symbols x 491,400 bars, the config-5 grid), 64 lanes in list mode, arena rows:
    M      tail_risk(lanes); MR the records alone; MH the host route on the same 64 lanes, whole.

The device's figures of the host route's lanes are compared with the host's, field by field.

    python scripts/tail_time.py [--out profiles/tail/tail_time.json] [--rounds 5] [--host-lanes 4096] [--skip-minute]
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
LEVELS = (0.01, 0.05, 0.10)
PPM = (10_000, 50_000, 100_000)


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def records_only(e, lanes=None):
    """bt_tail with q_out = NULL: the walk and the sums, no selection."""
    f = D.engine.sym("bt_tail")
    lv = np.array(PPM, np.int32)
    if lanes is None:
        n, req = e.stats()["n_symbols"] * e.n_params, None
    else:
        req = D.engine.as_lanes(lanes)
        n = len(req)
    out = np.zeros(n, D.TAIL_DTYPE)
    rc = f(e._h, 0 if req is None else n, None if req is None else req.ctypes.data, 0, 0, 0, len(lv), lv.ctypes.data,
           out.ctypes.data, None)
    assert rc == 0, D.lib().bt_last_error().decode()
    return out


def host_route(e, lanes):
    """(n, s1, s2, s3, s4, min, max, [(var, es_sum)]) per lane from replayed curves, on the host."""
    rp = e.replay(lanes, curves=True)
    out = []
    for i in range(len(lanes)):
        d = np.diff(rp.equity[i, :rp.n_bars[i]], prepend=0)
        n = len(d)
        x = [int(v) for v in d[d != 0]]
        qs = []
        for a in PPM:
            k = -(-n * a // 1_000_000)
            part = np.partition(d, k - 1)[:k]
            qs.append((int(part[k - 1]), int(part.sum())))
        out.append((n, int(d.sum()), sum(v * v for v in x), sum(v ** 3 for v in x), sum(v ** 4 for v in x),
                    int(d.min()), int(d.max()), qs))
    return out


def check_against_host(tr, ref):
    """The first len(ref) lanes of a result against the host route's figures, field by field."""
    n = len(ref)
    sub = D.TailRisk(tr.levels_ppm, tr.lanes.reshape(-1)[:n], tr.quantiles.reshape(-1, len(PPM))[:n])
    s2, s3, s4 = sub.s2, sub.s3, sub.s4          # each builds its Python ints once
    for i, h in enumerate(ref):
        r, q = sub.lanes[i], sub.quantiles[i]
        dev = (int(r["n"]), int(r["s1"]), s2[i], s3[i], s4[i], int(r["min_d"]), int(r["max_d"]),
               [(int(x["var"]), int(x["es_sum"])) for x in q])
        assert dev == h, (i, dev, h)


def stats(ts):
    return {"median_ms": round(statistics.median(ts) * 1e3, 3), "min_ms": round(min(ts) * 1e3, 3),
            "max_ms": round(max(ts) * 1e3, 3), "samples_ms": [round(t * 1e3, 3) for t in ts]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-lanes", type=int, default=4096)
    ap.add_argument("--skip-minute", action="store_true")
    args = ap.parse_args()
    res = {}
    grid = D.config2_grid()
    P = grid.n_params
    with D.Engine(grid) as e:
        e.load_synthetic(0xD1CE, SYM_BEGIN, N_SYM, BARS, D.BT_DAILY)
        t = {1: [], 2: []}
        for row in (1, 2):         # warm-up of both homes (the arena grows here)
            e.set_tail_row(row)
            e.tail_risk(LEVELS)
        for _ in range(args.rounds):
            for row in (1, 2):
                e.set_tail_row(row)
                dt, tr = clock(lambda: e.tail_risk(LEVELS))
                assert e.last_tail_row() == row
                t[row].append(dt)
                if row == 1:
                    lds = tr
                else:
                    assert tr.lanes.tobytes() == lds.lanes.tobytes() and tr.quantiles.tobytes() == lds.quantiles.tobytes()
        print(json.dumps({"lds_row": stats(t[1]), "arena_row": stats(t[2])}), flush=True)
        e.set_tail_row(1)
        records_only(e)
        t_r = [clock(lambda: records_only(e))[0] for _ in range(3)]
        e.set_tail_row(0)
        default_home = (e.tail_risk(LEVELS), e.last_tail_row())[1]
        n = min(args.host_lanes, D.REPLAY_MAX, N_SYM * P)
        lanes = [(SYM_BEGIN + i // P, i % P) for i in range(n)]
        host_route(e, lanes[:64])  # warm-up
        t_h, ref = clock(lambda: host_route(e, lanes))
        check_against_host(lds, ref)
        scale = N_SYM * P / n
        res["config2_shard"] = {
            "symbols": N_SYM, "bars": BARS, "params": P, "lanes": N_SYM * P, "levels_ppm": list(PPM),
            "lds_row": stats(t[1]), "arena_row": stats(t[2]), "records_only_lds": stats(t_r),
            "selection_share_of_the_call": round(1.0 - statistics.median(t_r) / statistics.median(t[1]), 3),
            "planner_home": default_home,
            "bytes_to_host": N_SYM * P * (D.TAIL_DTYPE.itemsize + len(PPM) * D.TAIL_Q_DTYPE.itemsize),
            "host_route_lanes": n, "host_route_ms": round(t_h * 1e3, 1), "scale": round(scale, 3),
            "host_route_scaled_ms": round(t_h * 1e3 * scale, 1), "lanes_checked_against_the_route": n,
        }
        print(json.dumps(res), flush=True)
    if not args.skip_minute:
        grid = D.config5_grid()
        P = grid.n_params
        with D.Engine(grid) as e:
            e.load_synthetic(0xD1CE, SYM_BEGIN, 8, 491_400, D.BT_MINUTE)
            lanes = [(SYM_BEGIN + i % 8, (i * 37) % P) for i in range(64)]
            e.tail_risk(LEVELS, lanes)
            t_m = [clock(lambda: e.tail_risk(LEVELS, lanes)) for _ in range(3)]
            home = e.last_tail_row()
            records_only(e, lanes)
            t_mr = [clock(lambda: records_only(e, lanes))[0] for _ in range(3)]
            t_h, ref = clock(lambda: host_route(e, lanes))
            check_against_host(t_m[0][1], ref)
        res["minute_rows"] = {
            "symbols": 8, "bars": 491_400, "lanes": 64, "row_home": home, "tail_risk": stats([x[0] for x in t_m]),
            "records_only": stats(t_mr),
            "selection_share_of_the_call": round(1.0 - statistics.median(t_mr) / statistics.median([x[0] for x in t_m]), 3),
            "host_route_ms": round(t_h * 1e3, 1), "lanes_checked_against_the_route": 64,
        }
        print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
