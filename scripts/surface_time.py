"""Time bt_surface (the run's summaries reduced on the GPU) against the route to the same figures
without it: Engine.summaries(), which copies the whole S x P matrix to the host, followed by a
vectorised numpy reduction of the same fields, and against the byte model of the reduction
(S*P*48 B read once plus the partial buffers written and read back, over the 6.29 TB/s the
microarchitecture guide measured for a device copy).

Shapes: the full configs 2, 3 and 4 and the 1,250-symbol shard of config 5. Each engine runs its
sweep once; bt_surface is then called once to warm up (it allocates its partial buffers) and
timed with host clocks around the synchronous call: the median of 9 samples of 200 calls back to
back, reported per call. The call waits for its kernels
and copies P x 104 B + S x 24 B back, so the figure holds the launch, the wait and that copy as
well as the kernels; an empty bt_sync on the idle engine is timed the same way as the floor of
the host-side cost. The numpy route's result is compared with the device's, byte for byte.

    python scripts/surface_time.py [--out profiles/surface/surface_time.json] [--cases config2,config3]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dbx_amd as D  # noqa: E402
from dbx_amd import engine as E  # noqa: E402

COPY_RATE = 6.29e12  # B/s, device copy rate measured on the MI355X
CASES = {
    "config2": (D.config2_grid, 5000, 2520, D.BT_DAILY),
    "config3": (D.config3_grid, 500, 98_280, D.BT_MINUTE),
    "config4": (D.config4_grid, 500, 98_280, D.BT_MINUTE),
    "config5_shard": (D.config5_grid, 1250, 491_400, D.BT_MINUTE),
}


def timed(fn, repeats=9, inner=1):
    """Median over `repeats` samples of the time per call, each sample `inner` calls back to back
    (the synchronous device calls take tens of microseconds: a sample of 200 is ~15 ms)."""
    fn()  # warm-up
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(inner):
            out = fn()
        ts.append((time.perf_counter() - t0) / inner)
    return statistics.median(ts), out


def numpy_surface(m, ids):
    """The reductions of docs/surface_spec.md in vectorised numpy (exact: the 128-bit sums are
    assembled from int64 column sums of 24-bit limbs, which fit while S < 2^15)."""
    S, P = m.shape
    assert 0 < S < 2**15
    ok = m["status"] == 0
    sh = m["sharpe"]
    out = np.zeros(P, D.PARAM_AGG_DTYPE)
    out["n_sym"] = ok.sum(0)
    out["n_traded"] = (ok & (m["n_trades"] > 0)).sum(0)
    out["n_win"] = (ok & (m["pnl"] > 0)).sum(0)
    out["n_pos"] = (ok & (sh > 0)).sum(0)
    for f, g in (("trades", "n_trades"), ("pnl", "pnl"), ("exposure", "exposure")):
        out[f] = np.where(ok, m[g], 0).sum(0, dtype=np.int64)
    any_ = out["n_sym"] > 0
    out["mdd_max"] = np.where(any_, np.where(ok, m["mdd"], np.iinfo(np.int64).min).max(0, initial=np.iinfo(np.int64).min), 0)
    bits = sh.view(np.uint64)
    key = np.where(bits >> np.uint64(63) != 0, ~bits, bits | np.uint64(1 << 63))
    big = np.iinfo(np.int64).max
    idcol = np.asarray(ids, np.int64)[:, None]
    for name, pick, fill in (("max", np.max, np.uint64(0)), ("min", np.min, np.uint64(2**64 - 1))):
        k = pick(np.where(ok, key, fill), axis=0, initial=fill)
        hit = ok & (key == k)
        out["sym_" + name] = np.where(any_, np.where(hit, idcol, big).min(0, initial=big), -1)
        row = np.argmax(hit, axis=0)
        out["sharpe_" + name] = np.where(any_, sh[row, np.arange(P)], 0.0)
    q = np.rint(np.clip(np.where(sh == sh, sh, 0.0), -32768.0, 32768.0) * 2.0**32).astype(np.int64)
    q = np.where(ok, q, 0)
    hi, lo = q >> 24, q & ((1 << 24) - 1)      # q = hi 2^24 + lo, |hi| <= 2^23
    s1 = q.sum(0, dtype=np.int64)
    hh, hl, ll = (hi * hi).sum(0, dtype=np.int64), (hi * lo).sum(0, dtype=np.int64), (lo * lo).sum(0, dtype=np.int64)
    for p in range(P):
        for name, v in (("ss1", int(s1[p])), ("ss2", (int(hh[p]) << 48) + (int(hl[p]) << 25) + int(ll[p]))):
            u = v & ((1 << 128) - 1)
            out[name + "_lo"][p] = u & (2**64 - 1)
            h = u >> 64
            out[name + "_hi"][p] = h - 2**64 if h >> 63 else h
    best = np.zeros(S, D.TOPK_DTYPE)
    bp = np.argmax(key, axis=1)                # the first of equal keys: the lowest param
    rows = np.arange(S)
    best["sharpe"], best["sym"], best["param"], best["pnl"] = sh[rows, bp], ids, bp, m["pnl"][rows, bp]
    return out, best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default=",".join(CASES))
    args = ap.parse_args()
    plan_exe = None
    res = {}
    for name in args.cases.split(","):
        mk, n_sym, bars, freq = CASES[name]
        grid = mk()
        P = grid.n_params
        with D.Engine(grid) as e:
            e.load_synthetic(0xD1CE, 1000, n_sym, bars, freq)
            e.run()
            e.sync()
            f, sync = E.sym("bt_surface"), D.lib().bt_sync
            agg = np.zeros(P, D.PARAM_AGG_DTYPE)
            best = np.zeros(n_sym, D.TOPK_DTYPE)
            t_sync, _ = timed(lambda: sync(e._h), inner=200)
            t_both, rc = timed(lambda: f(e._h, agg.ctypes.data, best.ctypes.data), inner=200)
            assert rc == 0
            t_agg, rc = timed(lambda: f(e._h, agg.ctypes.data, None), inner=200)
            assert rc == 0
            assert f(e._h, agg.ctypes.data, best.ctypes.data) == 0   # both outputs for the comparison below
            t_read, m = timed(lambda: e.summaries(), repeats=3)
            ids = np.arange(1000, 1000 + n_sym, dtype=np.int32)
            t_np, (np_agg, np_best) = timed(lambda: numpy_surface(m, ids), repeats=3)
            assert np_agg.tobytes() == agg.tobytes(), name
            assert np_best.tobytes() == best.tobytes(), name
            cus = __import__("torch").cuda.get_device_properties(0).multi_processor_count
        # the chunk count the planner chose for this device (tests/plan/surface_plan_driver.cpp)
        if plan_exe is None:
            import tempfile
            csrc = os.path.join(ROOT, "distributed-backtesting-exploration_amd", "csrc")
            plan_exe = os.path.join(tempfile.mkdtemp(prefix="bt_splan_"), "surface_plan_driver")
            subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-x", "hip", "--cuda-host-only", "-I", csrc,
                            "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "plan", "surface_plan_driver.cpp"),
                            os.path.join(csrc, "plan.cpp"), "-o", plan_exe], check=True)
        pl = json.loads(subprocess.run([plan_exe, str(n_sym), str(P), str(cus), "0"], capture_output=True,
                                       text=True, check=True).stdout)
        model_bytes = n_sym * P * 48 + 2 * pl["partial_bytes"] + 2 * pl["best_partial_bytes"] + P * 104 + n_sym * 24
        model_s = model_bytes / COPY_RATE
        res[name] = {
            "symbols": n_sym, "params": P, "matrix_bytes": n_sym * P * 48, "cus": cus, "chunks": pl["chunks"],
            "rows_per_chunk": pl["rows_per_chunk"], "block": pl["block"], "p_blocks": pl["p_blocks"],
            "surface_ms": round(t_both * 1e3, 4), "surface_agg_only_ms": round(t_agg * 1e3, 4),
            "idle_sync_ms": round(t_sync * 1e3, 4),
            "byte_model_bytes": model_bytes, "byte_model_ms": round(model_s * 1e3, 4),
            "fraction_of_byte_model": round(model_s / t_both, 4),
            "fraction_of_byte_model_less_sync": round(model_s / max(t_both - t_sync, 1e-9), 4),
            "readback_ms": round(t_read * 1e3, 3), "numpy_reduce_ms": round(t_np * 1e3, 3),
            "readback_route_over_surface": round((t_read + t_np) / t_both, 1),
        }
        print(json.dumps({name: res[name]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            json.dump(res, fo, indent=1)
            fo.write("\n")


if __name__ == "__main__":
    main()
