"""Run overlap without a GPU: the planner's decision (LaunchPlan::overlap of csrc/plan.cpp, through
tests/plan/overlap_plan_driver.cpp) and the switch's place in the ABI (bt_set_run_overlap).

A run may execute beside its neighbours exactly when it touches nothing single-buffered, the
engine owns its streams and there is a last round of blocks for the next run to fill: one bar
segment per symbol, no parity outputs, no profiling stamps (the release library has none), the
engine's own stream, the switch left on, and more blocks than the device holds at once. The last
condition is measured, not assumed: config 3's 500-symbol shard is one round of two blocks per CU
and ran 2.3 % slower overlapped (profiles/r11/run_overlap_ab.txt), so such a run stays serial."""
import itertools
import os
import re
import subprocess

import pytest

import dbx_amd as D
from dbx_amd import engine as E
from helpers import build_plan_driver, launch_plan, run_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = 256

# bench.py's four configurations at their one-GPU default shards: grid, symbols, bars
BENCH = {
    2: (D.config2_grid, 5000, 2520),
    3: (D.config3_grid, 500, 98280),
    4: (D.config4_grid, 2000, 98280),
    5: (D.config5_grid, 10000, 491400),
}


def overlap_plan(grid, n_sym, bars, cus=CUS, **kw):
    name = {D.BT_SMA_CROSS: "sma", D.BT_EMA_OLS: "ema_ols", D.BT_BOLL: "boll"}[grid.strategy]
    args = [name] + [f"{k}={','.join(str(int(v)) for v in a)}" for k, a in zip("abcd", grid.axes)]
    args += [f"band_bps={grid.band_bps}", f"k_den={grid.k_den}", f"sym={n_sym}", f"bars={bars}", f"cus={cus}"]
    args += [f"{k}={int(v)}" for k, v in kw.items()]
    return run_driver(build_plan_driver("overlap_plan_driver"), *args)


def test_overlap_is_true_only_when_every_condition_holds():
    grid = D.config2_grid()
    for parity, own, on, seg in itertools.product((0, 1), (0, 1), (0, 1), (0, 1, 2, 4)):
        got = overlap_plan(grid, 1600, 1000, parity=parity, own=own, on=on, seg=seg)
        want = got["G"] == 1 and not parity and own and on
        assert bool(got["overlap"]) == bool(want), (parity, own, on, seg, got)
    # each single reason on its own, and none
    assert overlap_plan(grid, 1600, 1000)["overlap"] == 1
    assert overlap_plan(grid, 1600, 1000, default=1) == overlap_plan(grid, 1600, 1000)
    split = overlap_plan(grid, 1600, 1000, seg=2)
    assert split == {"G": 2, "overlap": 0}
    assert overlap_plan(grid, 1600, 1000, parity=1)["overlap"] == 0
    assert overlap_plan(grid, 1600, 1000, own=0)["overlap"] == 0
    assert overlap_plan(grid, 1600, 1000, on=0)["overlap"] == 0
    # a parity run never splits, and never overlaps either
    assert overlap_plan(grid, 1600, 1000, parity=1, seg=2) == {"G": 1, "overlap": 0}


@pytest.mark.parametrize("config", sorted(BENCH))
def test_overlap_of_the_benchmark_configurations(config):
    make, n_sym, bars = BENCH[config]
    grid = make()
    got = overlap_plan(grid, n_sym, bars)
    # the segment count is the one the run planner reports for the same shard
    assert got["G"] == launch_plan(grid, n_sym=n_sym, bars=bars, cus=CUS)["G"]
    # more blocks than the device holds at once? A CU has 32 wave slots and 160 KB of LDS: config
    # 2's 8-wave blocks fit at most four to a CU, the tile kernels' 8-wave blocks two (LDS), config
    # 5's 16-wave blocks two; every grid here is one block per symbol
    per_cu = {2: 4, 3: 2, 4: 2, 5: 2}[config]
    assert launch_plan(grid, n_sym=n_sym, bars=bars, cus=CUS)["grid_y"] == 1
    assert got == {"G": 1, "overlap": int(n_sym > per_cu * CUS)}
    assert got["overlap"] == {2: 1, 3: 0, 4: 1, 5: 1}[config]
    for off in (dict(on=0), dict(own=0), dict(parity=1)):
        assert overlap_plan(grid, n_sym, bars, **off)["overlap"] == 0, off


def test_a_single_round_of_blocks_does_not_overlap():
    # config 2's grid: 8-wave blocks, one per symbol, at most four to a CU by wave slots alone
    grid = D.config2_grid()
    assert overlap_plan(grid, 4 * CUS + 1, 1000)["overlap"] == 1
    for n_sym in (1, 3, CUS, 2 * CUS):
        assert overlap_plan(grid, n_sym, 1000) == {"G": 1, "overlap": 0}, n_sym
    # the same shard on a smaller device is several rounds
    assert overlap_plan(grid, 2 * CUS, 1000, cus=64)["overlap"] == 1
    # config 3: two 8-wave blocks of 80.2 KB to a CU
    ema = D.config3_grid()
    assert overlap_plan(ema, 2 * CUS, 98280, seg=1) == {"G": 1, "overlap": 0}
    assert overlap_plan(ema, 2 * CUS + 1, 98280, seg=1) == {"G": 1, "overlap": 1}


def test_small_shards_that_split_do_not_overlap():
    # config 3 on two GPUs, config 4 on eight and config 5's per-GPU shard: automatic
    # bar segments, whose records are single-buffered
    for make, n_sym, bars in ((D.config3_grid, 250, 98280), (D.config4_grid, 250, 98280),
                              (D.config5_grid, 1250, 491400)):
        grid = make()
        got = overlap_plan(grid, n_sym, bars)
        assert got["G"] == launch_plan(grid, n_sym=n_sym, bars=bars, cus=CUS)["G"] > 1
        assert got["overlap"] == 0
        assert overlap_plan(grid, n_sym, bars, seg=1)["G"] == 1


def test_overlap_driver_under_asan_and_ubsan():
    grid = D.config2_grid()
    name = "overlap_plan_driver"
    args = ["sma"] + [f"{k}={','.join(str(int(v)) for v in a)}" for k, a in zip("ab", grid.axes)]
    for extra in (["sym=1600", "bars=1000", "cus=256"], ["sym=3", "bars=300", "cus=256", "parity=1"],
                  ["sym=1250", "bars=491400", "cus=256", "on=0"]):
        assert run_driver(build_plan_driver(name, sanitize=True), *args, *extra, sanitized=True) == \
            run_driver(build_plan_driver(name), *args, *extra)


def test_switch_is_declared_exported_and_bound_late_at_abi_3():
    hdr = open(os.path.join(ROOT, "include", "bt.h")).read()
    assert re.search(r"^int32_t bt_set_run_overlap\(bt_engine\* e, int32_t on\);$", hdr, re.M)
    assert int(re.search(r"#define BT_ABI_VERSION (\d+)", hdr).group(1)) == 3 == D.ABI_VERSION
    out = subprocess.run(["nm", "-D", "--defined-only", E.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert re.search(r" T bt_set_run_overlap$", out, re.M)
    min_abi, argtypes, restype = E._LATE_SYMBOLS["bt_set_run_overlap"]
    assert min_abi == 3 and len(argtypes) == 2 and restype is not None
    f = E.sym("bt_set_run_overlap")
    assert f.argtypes == argtypes and f.restype is restype
    # a null engine is refused through the ABI's one error path, for either setting
    for on in (0, 1):
        assert f(None, on) == -1
        assert "bt_set_run_overlap: null engine" in D.lib().bt_last_error().decode()
    assert callable(D.Engine.set_run_overlap)
