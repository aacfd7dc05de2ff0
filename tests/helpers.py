"""Shared test helpers: oracle-vs-engine comparison (tests only)."""
import atexit
import functools
import json
import os
import shutil
import subprocess
import tempfile

import numpy as np

import dbx_amd as D
import orc_ffi as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def oracle_row(strategy, grid, ohlc, ann, cap=0):
    """Run the C oracle for every param of `grid` on one symbol; returns (summaries, trades)."""
    o, h, lo, c = ohlc
    out, trades = [], []
    for p in range(grid.n_params):
        kw = grid.param(p)
        if strategy == "sma":
            s, tr = F.sma(c, kw["f"], kw["s"], ann, cap)
        elif strategy == "ema_ols":
            s, tr = F.ema_ols(c, kw["n"], kw["w"], kw["band_bps"], ann, cap)
        else:
            s, tr = F.boll(h, lo, c, kw["w"], kw["k_num"], kw["k_den"], kw["sl"], kw["tp"], ann, cap)
        out.append(s)
        trades.append(tr)
    return out, trades


FIELDS = ("n_trades", "pnl", "mdd", "exposure", "hash")


def compare_summary(gpu, orc, where=""):
    """Bit-exact comparison of one engine summary vs one oracle summary."""
    for f in FIELDS:
        assert int(gpu[f]) == int(orc[f]), f"{where}: {f} gpu={gpu[f]} oracle={orc[f]}"
    # Sharpe: bit-exact by construction (exact int128 sums, fixed op sequence); the north_star
    # tolerance (1e-9 relative) is asserted as well so a failure message shows the size.
    g, o = float(gpu["sharpe"]), float(orc["sharpe"])
    assert abs(g - o) <= 1e-9 * max(abs(o), 1e-300), f"{where}: sharpe {g!r} vs {o!r}"
    assert g == o, f"{where}: sharpe not bit-exact {g!r} vs {o!r}"


def compare_summaries(gpu, orc, where):
    """Bit-exact comparison of two equal-shape summary arrays (every field, Sharpe by bits);
    the first mismatch is reported through compare_summary with where(index)."""
    assert gpu.shape == orc.shape, f"shapes {gpu.shape} vs {orc.shape}"
    bad = np.zeros(gpu.shape, dtype=bool)
    for f in FIELDS:
        bad |= gpu[f].astype(np.int64) != orc[f].astype(np.int64)
    bad |= gpu["sharpe"].astype(np.float64).view(np.uint64) != orc["sharpe"].astype(np.float64).view(np.uint64)
    if bad.any():
        i = tuple(int(x) for x in np.argwhere(bad)[0])
        compare_summary(gpu[i], orc[i], where(i))
        raise AssertionError(f"{where(i)}: summaries differ")


def compare_trades(gpu_tr, orc_tr, n, where=""):
    got = [tuple(int(x) for x in (t["entry_bar"], t["exit_bar"], t["side"], t["entry_px"], t["exit_px"]))
           for t in gpu_tr[:n]]
    exp = [tuple(int(x) for x in (t["entry_bar"], t["exit_bar"], t["side"], t["entry_px"], t["exit_px"]))
           for t in orc_tr[:n]]
    assert got == exp, f"{where}: trade lists differ (first diff at {next((i for i,(a,b) in enumerate(zip(got,exp)) if a!=b), None)})"


CSRC = os.path.join(ROOT, "distributed-backtesting-exploration_amd", "csrc")
SANITIZE = ("-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
            "-Xarch_host", "-fno-omit-frame-pointer")
# verify_asan_link_order=0: the environment may preload a library ahead of the ASan runtime
SANITIZE_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0")


@functools.lru_cache(None)
def build_plan_driver(name, sources=("plan.cpp",), sanitize=False):
    """tests/plan/<name>.cpp and the given csrc files built once per session, the way the Makefile
    compiles host files (host pass only: the planner makes no HIP call and needs no GPU);
    `sanitize`: as a stand-alone program under AddressSanitizer and UBSan."""
    exe = os.path.join(tempfile.mkdtemp(prefix="bt_plan_"), name)
    atexit.register(shutil.rmtree, os.path.dirname(exe), True)
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror",
                        *(SANITIZE if sanitize else ()), "-x", "hip", "--cuda-host-only", "-I", CSRC,
                        "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "plan", name + ".cpp"),
                        *(os.path.join(CSRC, s) for s in sources), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_driver(exe, *args, sanitized=False):
    """One JSON line from a plan driver."""
    r = subprocess.run([exe, *(str(a) for a in args)], capture_output=True, text=True, timeout=120,
                       env=SANITIZE_ENV if sanitized else None)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return json.loads(r.stdout)


def assert_staging_layout(regions, staging_bytes, where=""):
    """The rule of every analysis plan (csrc/plan.h): the regions, [(offset, bytes)] in layout
    order, start on 256-byte boundaries, follow each other without overlap and end inside
    staging_bytes, which is never below 256."""
    end = 0
    for i, (off, size) in enumerate(regions):
        assert off % 256 == 0 and off >= end, f"{where}: region {i} at {off} after {end}"
        end = off + size
    assert max(end, 256) <= staging_bytes, f"{where}: regions end at {end}, staging {staging_bytes}"


def _plan_driver():
    return build_plan_driver("plan_driver")


@functools.lru_cache(None)
def _plan(args):
    out = subprocess.run([_plan_driver(), *args], capture_output=True, text=True, check=True).stdout
    return json.loads(out)


def launch_plan(grid, n_sym=1, bars=64, cus=256, parity=False, seg=0, burn=0):
    """What the library launches for `grid` on a shard of n_sym symbols of at most `bars` bars on a
    device of `cus` compute units: the real planner (csrc/plan.cpp, through tests/plan/plan_driver),
    as a dict of the grid's ring and the LaunchPlan fields. "ema_lds" holds an EMA+OLS block's LDS
    bytes at 64-bar and at 128-bar stages, "ts" the stage the launcher picks."""
    name = {D.BT_SMA_CROSS: "sma", D.BT_EMA_OLS: "ema_ols", D.BT_BOLL: "boll"}[grid.strategy]
    args = [name] + [f"{k}={','.join(str(int(v)) for v in a)}" for k, a in zip("abcd", grid.axes)]
    args += [f"band_bps={grid.band_bps}", f"k_den={grid.k_den}", f"sym={n_sym}", f"bars={bars}",
             f"cus={cus}", f"parity={int(parity)}", f"seg={seg}", f"burn={burn}"]
    return dict(_plan(tuple(args)))


def gpu_cus():
    """Compute units of GPU 0 (GPU tests: the CU count the engine plans with)."""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count
