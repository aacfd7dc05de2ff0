"""CPU side of the lane replay (bt_replay, Engine.replay): the numpy curve reconstruction the GPU
tests compare against is pinned to the C oracle's own fields, the entry point is declared and
bound, the Python surface exists, every accepted form of `lanes` gives the same request, and what
the call decides on the host (plan_replay of csrc/plan.cpp, the rules of csrc/replay.cpp) through
tests/plan/replay_plan_driver.cpp, once more under AddressSanitizer and UBSan."""
import os
import re

import numpy as np
import pytest

import dbx_amd as D
from dbx_amd import engine as E
from helpers import assert_staging_layout, build_plan_driver, run_driver
from replay_ref import curves_from_trades, gen_hlc, oracle_lane

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GRIDS = {
    "sma": D.Grid.sma([3, 10], [7, 40], annualization=98280),
    "ema_ols": D.Grid.ema_ols([5, 30], [4, 50], band_bps=5),
    "boll": D.Grid.boll([5, 40], [2, 3], [30], [60], k_den=2),
}


@pytest.mark.parametrize("strategy", list(GRIDS))
@pytest.mark.parametrize("bars", [1, 2, 3, 64, 65, 1000])
def test_curve_reconstruction_matches_the_oracle_fields(strategy, bars):
    grid = GRIDS[strategy]
    h, lo, c = gen_hlc(0xC0FFEE, 17 + bars, bars, 1)
    traded = 0
    for p in range(grid.n_params):
        s, tr = oracle_lane(strategy, grid, p, (h, lo, c), cap=4096)
        assert int(s["n_trades"]) <= 4096
        pos, eq = curves_from_trades(c, tr)
        peak = np.maximum.accumulate(np.maximum(eq, 0))
        assert int((peak - eq).max()) == int(s["mdd"])
        assert int(eq[-1]) == int(s["pnl"])
        assert int(np.count_nonzero(pos[:-1])) == int(s["exposure"])
        assert pos[-1] == 0
        traded += int(s["n_trades"])
    if bars == 1000:
        assert traded >= 10 * grid.n_params


def test_bt_replay_is_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "bt.h")).read()
    assert re.search(r"int32_t\s+bt_replay\s*\(\s*bt_engine\*", hdr)
    assert re.search(r"#define BT_REPLAY_MAX (\d+)", hdr).group(1) == str(D.REPLAY_MAX)
    assert re.search(r"typedef struct bt_lane \{\s*int32_t sym;[^}]*int32_t param;[^}]*\} bt_lane;", hdr)
    assert int(re.search(r"#define BT_ABI_VERSION (\d+)", hdr).group(1)) == 3
    assert E._LATE_SYMBOLS["bt_replay"][0] == 3
    f = E.sym("bt_replay")
    assert f is not None and len(f.argtypes) == 10
    # a null engine is refused, not dereferenced
    assert f(None, 0, None, 0, None, None, None, None, None, 0) == -1
    assert "null engine" in D.lib().bt_last_error().decode()


def test_python_surface():
    assert callable(D.Engine.replay)
    assert D.LANE_DTYPE.names == ("sym", "param") and D.LANE_DTYPE.itemsize == 8
    assert {"lanes", "summaries", "n_bars", "trades", "equity", "pos"} <= set(D.Replay.__dataclass_fields__)
    for name in ("Replay", "LANE_DTYPE", "REPLAY_MAX", "as_lanes"):
        assert name in D.__all__


def test_lane_forms_give_the_same_request():
    top = np.zeros(5, D.TOPK_DTYPE)
    top["sym"] = [907, 12, 500, 12, 2**31 - 1]
    top["param"] = [3, 0, 11, 0, 7]
    top["sharpe"] = [2.5, 1.0, 0.5, 0.25, -1.0]
    top["pnl"] = [10, 20, 30, 40, 50]
    want = D.as_lanes(top)
    assert want.dtype == D.LANE_DTYPE and want.flags["C_CONTIGUOUS"]
    assert want["sym"].tolist() == top["sym"].tolist() and want["param"].tolist() == top["param"].tolist()
    pairs = [(int(s), int(p)) for s, p in zip(top["sym"], top["param"])]
    for form in (np.array(pairs, np.int64), np.array(pairs, np.int32), pairs, [list(x) for x in pairs],
                 iter(pairs), want, top[["sym", "param"]]):
        got = D.as_lanes(form)
        assert got.dtype == D.LANE_DTYPE and got.tobytes() == want.tobytes()
    assert len(D.as_lanes([])) == 0 and D.as_lanes([]).dtype == D.LANE_DTYPE
    assert len(D.as_lanes(np.zeros((0, 2), np.int64))) == 0
    for bad in ([(1, 2, 3)], [1, 2], np.zeros((2, 2), np.float64), [(2**31, 0)]):
        with pytest.raises(ValueError):
            D.as_lanes(bad)


# ------------------------------------------------------------------------------------ planner
BUDGET = 256 << 20
REPLAY_SOURCES = ("plan.cpp", "replay.cpp")


@pytest.fixture(scope="module")
def driver():
    exe = build_plan_driver("replay_plan_driver", REPLAY_SOURCES)
    return lambda *args: run_driver(exe, *args)


def _check_plan(pl, n, W, cap, stride, equity, pos, budget, where):
    assert pl["budget"] == BUDGET and (pl["lane_bytes"], pl["summary_bytes"], pl["trade_bytes"]) == (16, 48, 32)
    dcap, pitch = pl["dcap"], pl["pitch"]
    assert dcap == min(cap, W), where
    assert pitch == (min(stride, -(-W // 64) * 64) if equity or pos else 0), where
    per_lane = 16 + 48 + dcap * 32 + (pitch * 8 if equity else 0) + (pitch if pos else 0)
    L = pl["lanes_per_chunk"]
    assert L == min(n, max(1, (budget - 5 * 256) // per_lane)), where
    assert_staging_layout([(pl["o_lane"], L * 16), (pl["o_sum"], L * 48), (pl["o_trades"], L * dcap * 32),
                           (pl["o_equity"], L * pitch * 8 if equity else 0), (pl["o_pos"], L * pitch if pos else 0)],
                          pl["staging_bytes"], where)
    assert pl["o_lane"] == 0
    if 5 * 256 + per_lane <= budget:   # one lane alone fits: so does every chunk
        assert pl["staging_bytes"] <= budget, where
    # every lane exactly once
    assert pl["chunks"] == -(-n // L), where
    lanes = pl["lanes"]
    assert lanes[0][0] == 0 and lanes[-1][1] == n and all(0 < b - a <= L for a, b in lanes), where
    if pl["chunks"] <= 8:
        assert len(lanes) == pl["chunks"] and all(a[1] == b[0] for a, b in zip(lanes[:-1], lanes[1:])), where
    else:
        assert lanes[3] == [3 * L, 4 * L] and lanes[-1][0] == (pl["chunks"] - 1) * L, where
    return per_lane


@pytest.mark.parametrize("n", (1, 2, 4096))
def test_plan_replay_lays_out_every_chunk_within_the_budget(driver, n):
    one_lane_too_big = 0
    for W in (1, 64, 65, 100_000, 1 << 22):
        for cap in (0, 3, W + 5):
            stride = W if cap == 0 else -(-W // 64) * 64 + 64   # the shortest accepted, and past the row pitch
            for equity, pos in ((0, 0), (1, 0), (1, 1)):
                where = f"n {n} W {W} cap {cap} equity {equity} pos {pos}"
                pl = driver("plan", n, W, cap, stride, equity, pos, 0)
                assert pl == driver("plan", n, W, cap, stride, equity, pos, 0), "the plan is a function of its arguments"
                per_lane = _check_plan(pl, n, W, cap, stride, equity, pos, BUDGET, where)
                assert 5 * 256 + per_lane <= BUDGET, "one lane always fits the default budget"
                # small budgets that leave 1, 2 and n - 1 lanes per chunk
                for want in sorted({w for w in (1, 2, n - 1) if 1 <= w <= n}):
                    budget = 5 * 256 + want * per_lane + per_lane // 2
                    small = driver("plan", n, W, cap, stride, equity, pos, budget)
                    _check_plan(small, n, W, cap, stride, equity, pos, budget, f"{where} budget {budget}")
                    assert small["lanes_per_chunk"] == want and small["chunks"] == -(-n // want)
                    assert (small["dcap"], small["pitch"]) == (pl["dcap"], pl["pitch"])
                # a budget below one lane: still one lane per chunk, the only case past the budget
                tiny = driver("plan", n, W, cap, stride, equity, pos, per_lane)
                assert tiny["lanes_per_chunk"] == 1 and tiny["chunks"] == n
                one_lane_too_big += tiny["staging_bytes"] > per_lane
    assert one_lane_too_big


def test_plan_replay_on_the_chunked_shape_of_the_gpu_suite(driver):
    """1,024 lanes x 100,000 bars with both curves (test_gpu_replay.py): 298 lanes a chunk, 4 chunks."""
    pl = driver("plan", 1024, 100_000, 0, 100_000, 1, 1, 0)
    assert (pl["lanes_per_chunk"], pl["chunks"], pl["pitch"], pl["dcap"]) == (298, 4, 100_000, 0)
    assert pl["lanes"] == [[0, 298], [298, 596], [596, 894], [894, 1024]]
    assert pl["o_trades"] == pl["o_equity"] and pl["staging_bytes"] <= BUDGET
    assert driver("plan", 0, 0, 0, 0, 0, 0, 0)["chunks"] == 0


# ------------------------------------------------------------------------------------- rules
P = 4   # parameters of the engine the resolution is checked against


def _rules(driver):
    """Every refusal test_gpu_replay.py asserts on the device, and the accepted cases between."""
    refusal = lambda *a: driver("refusal", *a)["why"]
    resolve = lambda curves, stride, *lanes: driver("resolve", P, curves, stride, *(f"{s}:{p}" for s, p in lanes))
    return refusal, resolve


def _check_rules(refusal, resolve):
    #                have_dataset n trade_cap have_trades have_lanes have_sum
    assert refusal(0, 1, 0, 0, 1, 1) == "no dataset loaded"
    assert refusal(0, D.REPLAY_MAX + 1, -7, 0, 0, 0) == "no dataset loaded", "the first rule that fails speaks"
    assert refusal(1, D.REPLAY_MAX + 1, 0, 0, 1, 1) == f"n = {D.REPLAY_MAX + 1} outside [0, {D.REPLAY_MAX}]"
    assert refusal(1, -1, 0, 0, 1, 1) == f"n = -1 outside [0, {D.REPLAY_MAX}]"
    assert refusal(1, 1, -7, 0, 1, 1) == "trade_cap = -7 is negative"
    assert refusal(1, 2, 0, 1, 1, 1) == "trades given with trade_cap = 0"
    assert refusal(1, 2, 4, 0, 1, 1) == "trade_cap = 4 without a trades buffer"
    assert refusal(1, 2, 4, 1, 0, 1) == refusal(1, 2, 4, 1, 1, 0) == "lanes and sum are required"
    assert refusal(1, 0, 0, 0, 0, 0) == "", "nothing requested needs no buffers"
    assert refusal(1, 0, 3, 1, 0, 0) == "" and refusal(1, D.REPLAY_MAX, 4, 1, 1, 1) == ""
    # rows of 64, 65 and 1,000 bars with ids 907, 12, 907: the first row of a repeated id wins
    got = resolve(1, 65, (12, 0), (907, 3), (12, 3), (907, 0))
    assert got == {"why": "", "W": 65, "lanes": [[64, 65, 0], [0, 64, 3], [64, 65, 3], [0, 64, 0]]}
    assert resolve(1, 64, (907, 1)) == {"why": "", "W": 64, "lanes": [[0, 64, 1]]}
    assert resolve(0, 0, (12, 2))["why"] == "" and resolve(0, 0)["lanes"] == []
    assert resolve(0, 0, (907, 0), (999, 0))["why"] == "unknown symbol id 999 (lane 1)"
    assert resolve(0, 0, (907, P))["why"] == f"param {P} outside [0, {P}) (lane 0)"
    assert resolve(0, 0, (12, 0), (12, -1))["why"] == f"param -1 outside [0, {P}) (lane 1)"
    assert resolve(0, 0, (999, P))["why"] == "unknown symbol id 999 (lane 0)", "the id before the param"
    assert resolve(1, 64, (907, 0), (12, 0))["why"] == "stride = 64 shorter than the longest requested symbol (65 bars)"
    assert resolve(1, 0, (907, 0))["why"] == "stride = 0 shorter than the longest requested symbol (64 bars)"
    assert resolve(1, 0, (907, P))["why"].startswith("param "), "the lanes before the stride"


def test_refusals_and_resolution_word_for_word(driver):
    _check_rules(*_rules(driver))


def test_messages_are_the_ones_the_gpu_suite_matches(driver):
    """The patterns tests/test_gpu_replay.py and tests/test_gpu_lifecycle.py match on the device."""
    refusal, resolve = _rules(driver)
    for msg, named in (
        (refusal(0, 1, 0, 0, 1, 1), "no dataset"),
        (resolve(0, 0, (907, 0), (999, 0))["why"], "999"),
        (resolve(0, 0, (907, P))["why"], rf"param {P} "),
        (resolve(0, 0, (907, -1))["why"], "param -1 "),
        (refusal(1, D.REPLAY_MAX + 1, 0, 0, 1, 1), str(D.REPLAY_MAX + 1)),
        (refusal(1, 1, -7, 0, 1, 1), "-7"),
        (resolve(1, 64, (12, 0), (907, 0))["why"], "stride = 64 .*65 bars"),
        (resolve(1, 0, (12, 0), (907, 0))["why"], "stride = 0 "),
        (refusal(1, 2, 0, 1, 1, 1), "trade_cap = 0"),
        (refusal(1, 2, 4, 0, 1, 1), "trade_cap = 4 "),
        (resolve(0, 0, (907, P))["why"], rf"param {P} outside \[0, {P}\)"),
    ):
        assert re.search(named, msg), (named, msg)


def test_plan_driver_under_asan_and_ubsan():
    exe = build_plan_driver("replay_plan_driver", REPLAY_SOURCES, sanitize=True)
    run = lambda *args: run_driver(exe, *args, sanitized=True)
    _check_rules(*_rules(run))
    args = (4096, 65, 70, 192, 1, 1, 5 * 256 + 2 * (64 + 65 * 32 + 128 * 9))
    pl = run("plan", *args)
    assert pl == run_driver(build_plan_driver("replay_plan_driver", REPLAY_SOURCES), "plan", *args)
    assert pl["lanes_per_chunk"] == 2
