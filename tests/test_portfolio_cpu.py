"""Portfolio of chosen lanes, the parts that need no GPU (docs/portfolio_spec.md): bt_portfolio_host
against the reference of portfolio_ref.py byte for byte, its refusals, bt_portfolio_merge, the
magnitudes the no-wrap argument allows, the planner (plan_portfolio through
tests/plan/portfolio_plan_driver.cpp) and the host code as a stand-alone program under
AddressSanitizer and UBSan (tests/asan/portfolio_driver.cpp)."""
import os
import re
import subprocess

import numpy as np
import pytest

import dbx_amd as D
from dbx_amd import engine as E
import portfolio_ref as PR
import walkfwd_ref as R
from helpers import CSRC, ROOT, SANITIZE, SANITIZE_ENV, assert_staging_layout, build_plan_driver, run_driver

STRATEGIES = ("sma", "ema_ols", "boll")


def _host(curves, lanes, T, ann):
    eq, ps, nb = PR.curve_arrays(curves, max(len(e) for _, e in curves))
    return D.portfolio_host(eq, ps, nb, windows=np.stack([lanes["from_bar"], lanes["to_bar"]], 1), T=T,
                            annualization=ann)


# ---------------------------------------------------------- (a) the host restatement, byte for byte
@pytest.mark.parametrize("strategy", STRATEGIES)
def test_host_equals_the_reference_on_the_edge_set(strategy):
    grid, lanes, curves, trades = PR.edge_entries(strategy)
    assert grid.n_params == 12 and len(lanes) == 2 * 9 * 12 + 12 + 6
    # the windows the case is there for, from the request and the oracle's trade lists alone
    windows = {(int(a), int(b)) for a, b in zip(lanes["from_bar"], lanes["to_bar"])}
    assert windows == set(PR.WINDOWS) | set(PR.MID_WINDOWS) | {(0, PR.WHOLE)}
    assert PR.begins_inside_a_trade(lanes, trades) >= 3
    assert len(lanes) - len(np.unique(lanes)) >= 3, "entries given twice"
    for T in (1000, 130):
        want = PR.edge_reference(strategy, T)
        got = _host(curves, lanes, T, grid.annualization)
        PR.assert_equal(got, want, f"{strategy} T {T}")
        s = want[4]
        assert int(s["n_lanes"]) < len(lanes), "empty windows are not counted"
        assert int(s["first_bar"]) == 0 and int(s["n_bars"]) == T and int(s["max_gross"]) >= 3
        assert np.array_equal(got.gross(), got.n_long + got.n_short) and np.array_equal(got.net(), got.n_long - got.n_short)
        assert int(got.equity[-1]) == int(s["pnl"]) and float(s["sharpe"]) != 0.0


def test_windows_telescope_and_bars_outside_every_window_are_zero():
    grid, lanes, curves, _ = PR.edge_entries("sma")
    i = next(i for i, L in enumerate(lanes) if (int(L["from_bar"]), int(L["to_bar"])) == (100, 700) and len(curves[i][1]) == 1000)
    pos, eq = curves[i]
    got = _host([curves[i]], lanes[i:i + 1], 1000, grid.annualization)
    assert not got.pnl[:100].any() and not got.pnl[700:].any() and not got.n_long[700:].any()
    assert int(got.pnl.sum()) == eq[699] - eq[99] == int(got.summary["pnl"])
    assert (int(got.summary["first_bar"]), int(got.summary["n_bars"]), int(got.summary["n_lanes"])) == (100, 600, 1)
    assert int(got.summary["exposure"]) == sum(1 for t in range(100, 700) if pos[t])
    # no entry at all, and entries whose windows are all empty: zero rows and the zero summary
    for none in (D.portfolio_host(np.zeros((0, 4), np.int64), np.zeros((0, 4), np.int8), [], T=7),
                 _host([curves[i]], np.array([(1, 0, 5, 5)], D.PF_LANE_DTYPE), 7, 252)):
        assert len(none.pnl) == 7 and not none.pnl.any() and not none.equity.any() and not none.n_short.any()
        assert not none.summary.tobytes().strip(b"\0")


# -------------------------------------------------------------------------------- (b) refusals
def test_refusals_name_the_value_and_leave_the_library_usable():
    grid, lanes, curves, _ = PR.edge_entries("sma")
    want = PR.edge_reference("sma", 130)
    eq, ps, nb = PR.curve_arrays(curves, 1000)
    n = len(lanes)
    host = E.sym("bt_portfolio_host")
    bufs = E._pf_bufs(130)
    out = [b.ctypes.data for b in bufs]

    def last():
        return D.lib().bt_last_error().decode()

    def still_good():
        assert host(n, eq.ctypes.data, ps.ctypes.data, nb.ctypes.data, 1000, lanes.ctypes.data, 130, grid.annualization, *out) == 0
        PR.assert_equal(E._pf_result(bufs, 130, grid.annualization), want, "after a refusal")

    def lanes_with(i, **kw):
        a = lanes.copy()
        for k, v in kw.items():
            a[k][i] = v
        return a

    neg, back = lanes_with(17, from_bar=-4), lanes_with(40, from_bar=9, to_bar=8)
    early = lanes_with(1, from_bar=-4)
    short = nb.copy()
    short[3] = 1001
    e, p, b, l = eq.ctypes.data, ps.ctypes.data, nb.ctypes.data, lanes.ctypes.data
    for args, named in (
        ((-1, e, p, b, 1000, l, 130, 252, *out), r"bt_portfolio_host: n = -1 outside \[0, 1048576\]"),
        (((1 << 20) + 1, e, p, b, 1000, l, 130, 252, *out), r"n = 1048577 outside"),
        ((n, e, p, b, 1000, None, 130, 252, *out), r"lanes are required"),
        ((n, e, p, b, 1000, l, 0, 252, *out), r"T = 0 outside \[1, 4194304\]"),
        ((n, e, p, b, 1000, l, (1 << 22) + 1, 252, *out), r"T = 4194305 outside"),
        ((n, e, p, b, 1000, l, 130, 252, None, None, None, None, None), r"pnl, equity, n_long, n_short and summary are all NULL"),
        ((n, e, p, b, 1000, l, 130, 0, *out), r"annualization = 0 is not positive"),
        ((n, None, p, b, 1000, l, 130, 252, *out), r"equity, pos and n_bars are required"),
        ((n, e, p, short.ctypes.data, 1000, l, 130, 252, *out), r"n_bars = 1001 outside \[0, stride = 1000\] \(entry 3\)"),
        # every n_bars is checked before any window: the later entry's n_bars is what is named
        ((n, e, p, short.ctypes.data, 1000, early.ctypes.data, 130, 252, *out), r"n_bars = 1001 outside \[0, stride = 1000\] \(entry 3\)"),
        ((n, e, p, b, 1000, neg.ctypes.data, 130, 252, *out), r"from_bar = -4 is negative \(entry 17\)"),
        ((n, e, p, b, 1000, back.ctypes.data, 130, 252, *out), r"to_bar = 8 is below from_bar = 9 \(entry 40\)"),
    ):
        assert host(*args) == -1
        assert re.search(named, last()), last()
        still_good()
    merge = E.sym("bt_portfolio_merge")
    pnl, _, nl, ns, summ = bufs
    m = (pnl.ctypes.data, nl.ctypes.data, ns.ctypes.data, summ.ctypes.data)
    for args, named in (
        ((0, 130, *m, 252, *out), r"bt_portfolio_merge: world = 0 is below 1"),
        ((1, 0, *m, 252, *out), r"T = 0 outside"),
        ((1, 130, None, *m[1:], 252, *out), r"pnl, n_long, n_short and summaries are required"),
        ((1, 130, *m, 252, None, None, None, None, None), r"are all NULL"),
        ((1, 130, *m, -1, *out), r"annualization = -1 "),
        ((1, 100, *m, 252, *out), r"part 0 covers bars \[0, 130\) of T = 100"),
    ):
        assert merge(*args) == -1
        assert re.search(named, last()), last()
    still_good()
    # the entry points that take an engine refuse a null one
    assert E.sym("bt_portfolio")(None, 0, None, 10, *out) == -1
    assert re.search(r"bt_portfolio: null engine", last()), last()
    assert E.sym("bt_set_portfolio_replicas")(None, 0) == -1
    assert re.search(r"bt_set_portfolio_replicas: null engine", last()), last()
    still_good()
    with pytest.raises(ValueError, match="windows"):
        D.portfolio_host(eq, ps, nb, windows=[(0, 1), (2, 3)])
    with pytest.raises(ValueError, match="n x stride"):
        D.portfolio_host(eq, ps[:5], nb)


# ----------------------------------------------------------------------------------- (c) merge
@pytest.mark.parametrize("strategy", STRATEGIES)
def test_disjoint_parts_merge_to_the_bytes_of_the_whole(strategy):
    grid, lanes, curves, _ = PR.edge_entries(strategy)
    ann = grid.annualization
    for T in (1000, 130):
        want = PR.edge_reference(strategy, T)
        for world in (2, 3):
            parts = [_host(curves[k::world], lanes[k::world], T, ann) for k in range(world)]
            PR.assert_equal(D.merge_portfolios(parts), want, f"{strategy} T {T}, {world} parts")
        # a part without an entry, and one whose only window is empty, change nothing
        empty = D.portfolio_host(np.zeros((0, 1), np.int64), np.zeros((0, 1), np.int8), [], T=T, annualization=ann)
        blank = _host(curves[:1], np.array([(0, 0, 5, 5)], D.PF_LANE_DTYPE), T, ann)
        halves = [_host(curves[:100], lanes[:100], T, ann), empty, _host(curves[100:], lanes[100:], T, ann), blank]
        PR.assert_equal(D.merge_portfolios(halves), want, f"{strategy} T {T}, with empty parts")
        PR.assert_equal(D.merge_portfolios([empty]), PR.portfolio([], T, ann), "an empty part alone")
    with pytest.raises(ValueError, match="differ"):
        D.merge_portfolios([parts[0], _host(curves[:1], lanes[:1], 7, ann)])


# ------------------------------------------------------------------------------ (d) magnitudes
def test_magnitudes_past_one_word():
    grid, _, lanes, curves, want = PR.magnitude_case()
    s = want[4]
    assert int(s["s2_hi"]) != 0, "s2 needs its high word"
    assert int(np.abs(want[0]).max()) > 2**32 and int(np.abs(want[1]).max()) > 2**32
    assert len(lanes) == 2 * 9 * PR.MAG_REPEAT and int(s["max_gross"]) > 300
    PR.assert_equal(_host(curves, lanes, 300, grid.annualization), want, "magnitude case")


# --------------------------------------------------------------------------------- (e) planner
@pytest.fixture(scope="module")
def plan():
    exe = build_plan_driver("portfolio_plan_driver")

    def run(n, T, cus=256, replicas=0, budget=0):
        return run_driver(exe, n, T, cus, replicas, budget)
    return run


def _regions(pl, n, T):
    R, pitch = pl["R"], pl["pitch"]
    return [(pl["o_lanes"], n * pl["lane_bytes"]), (pl["o_acc_pnl"], R * pitch * 8), (pl["o_acc_cnt"], R * pitch * 8),
            (pl["o_pnl"], T * 8), (pl["o_equity"], T * 8), (pl["o_long"], T * 4), (pl["o_short"], T * 4),
            (pl["o_sum"], pl["summary_bytes"])]


PLAN_SHAPES = {"config2": (5000, 2520), "config5": (64, 491400), "longest": (1 << 20, 1 << 22), "one": (1, 1),
               "none": (0, 130), "few": (5, 65), "odd": (6400, 2521)}


@pytest.mark.parametrize("name", list(PLAN_SHAPES))
def test_plan_portfolio_layout(plan, name):
    n, T = PLAN_SHAPES[name]
    pl = plan(n, T)
    assert pl == plan(n, T), "the plan is a function of its arguments"
    assert pl["lane_bytes"] == 24 and pl["summary_bytes"] == 80 and pl["acc_budget"] == 64 << 20 and pl["max_replicas"] == 64
    assert pl["pitch"] % 64 == 0 and T <= pl["pitch"] < T + 64 and pl["tiles"] == pl["pitch"] // 64
    assert_staging_layout(_regions(pl, n, T), pl["staging_bytes"], name)
    R = pl["R"]
    # the largest power of two that is at most 64, at most n, and fits the budget; at least 1
    assert R >= 1 and R & (R - 1) == 0 and R <= 64 and R <= max(n, 1)
    assert R == 1 or R * pl["pitch"] * 16 <= 64 << 20
    assert 2 * R > 64 or 2 * R > n or 2 * R * pl["pitch"] * 16 > 64 << 20
    assert pl["acc_bytes"] == 2 * R * pl["pitch"] * 8 and pl["o_acc_cnt"] == pl["o_acc_pnl"] + R * pl["pitch"] * 8
    assert pl["out_bytes"] == pl["o_sum"] + 80 - pl["o_pnl"]
    assert pl["finish_block"] % 64 == 0 and 64 <= pl["finish_block"] <= 1024 and pl["finish_block"] >= min(T, 1024)


def test_plan_portfolio_replicas_and_staging_on_the_shapes_of_the_issue(plan):
    assert plan(5000, 2520)["R"] == 64 and plan(64, 491400)["R"] == 8 and plan(1 << 20, 1 << 22)["R"] == 1
    assert plan(5000, 491400)["R"] == 8 and plan(3, 2520)["R"] == 2 and plan(0, 2520)["R"] == 1
    # staging is O(R T + n): beyond the descriptors it does not depend on n, and it is never n x T
    a, b = plan(64, 2520), plan(1 << 20, 2520)
    assert b["staging_bytes"] - a["staging_bytes"] == ((1 << 20) - 64) * 24
    assert {k: b[k] - b["o_acc_pnl"] for k in b if k.startswith("o_")}.items() >= \
        {k: a[k] - a["o_acc_pnl"] for k in ("o_acc_cnt", "o_pnl", "o_equity", "o_long", "o_short", "o_sum")}.items()
    assert b["staging_bytes"] < 64 * 2560 * 16 + (1 << 20) * 24 + 2520 * 24 + 4096
    assert plan(1 << 20, 1 << 22)["staging_bytes"] < (64 << 20) + (1 << 20) * 24 + (1 << 22) * 24 + 4096
    # a requested count is honoured up to 64 and halved until the accumulators fit
    assert plan(5000, 2520, replicas=1)["R"] == 1 and plan(5, 2520, replicas=64)["R"] == 64
    assert plan(5000, 2520, replicas=1000)["R"] == 64 and plan(5000, 2520, replicas=3)["R"] == 3
    assert plan(64, 491400, replicas=64)["R"] == 8 and plan(64, 1 << 22, replicas=64)["R"] == 1
    assert plan(5000, 2520, budget=2560 * 16 * 4)["R"] == 4
    assert plan(5000, 2520, cus=256)["fill"] == pytest.approx(5000 / 8192)


def test_plan_driver_under_asan_and_ubsan():
    exe = build_plan_driver("portfolio_plan_driver", sanitize=True)
    for args in ((6400, 2521, 256, 0, 0), (64, 491400, 304, 64, 0), (0, 1, 1, 0, 0)):
        assert run_driver(exe, *args, sanitized=True) == run_driver(build_plan_driver("portfolio_plan_driver"), *args)


# ---------------------------------------------------------------------- (f) under the sanitizers
def test_host_code_under_asan_and_ubsan(tmp_path):
    """csrc/portfolio.cpp and replay.cpp (the id rule it reuses) as a program of their own."""
    exe = str(tmp_path / "portfolio_asan")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", *SANITIZE,
                        "-x", "hip", "--cuda-host-only", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "asan", "portfolio_driver.cpp"), os.path.join(CSRC, "portfolio.cpp"),
                        os.path.join(CSRC, "replay.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    for strategy, T, parts in (("sma", 1000, 3), ("boll", 130, 2), ("ema_ols", 65, 7)):
        grid, lanes, curves, _ = PR.edge_entries(strategy)
        want = PR.edge_reference(strategy, T) if T != 65 else PR.portfolio(
            [(pos, eq, int(L["from_bar"]), int(L["to_bar"])) for (pos, eq), L in zip(curves, lanes)], T, grid.annualization)
        eq, ps, nb = PR.curve_arrays(curves, 1000)
        fin, fout = str(tmp_path / f"in_{strategy}"), str(tmp_path / f"out_{strategy}")
        with open(fin, "wb") as f:
            f.write(np.array([len(lanes), T, 1000, parts], np.int32).tobytes() + np.int64(grid.annualization).tobytes() +
                    lanes.tobytes() + nb.tobytes() + eq.tobytes() + ps.tobytes())
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, env=SANITIZE_ENV, timeout=120)
        assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
        raw = open(fout, "rb").read()
        one = T * 24 + 80
        assert len(raw) == 2 * one
        for k, what in ((0, "whole"), (1, f"{parts} parts merged")):
            b = raw[k * one:(k + 1) * one]
            got = D.Portfolio(np.frombuffer(b[:T * 8], np.int64), np.frombuffer(b[T * 8:T * 16], np.int64),
                              np.frombuffer(b[T * 16:T * 20], np.int32), np.frombuffer(b[T * 20:T * 24], np.int32),
                              np.frombuffer(b[T * 24:], D.PF_SUMMARY_DTYPE)[0], grid.annualization)
            PR.assert_equal(got, want, f"{strategy} T {T} {what} under the sanitizers")
        lines = r.stdout.splitlines()
        assert lines[-1] == f"ok {len(lanes)} {T} {parts}"
        refused = [ln for ln in lines if ln.startswith("refused: ")]
        assert len(refused) == 9
        for ln, named in zip(refused, ("n = -1 ", "n = 1048577 ", "T = 0 ", "T = 4194305 ", "all NULL", "annualization = 0 ",
                                       "from_bar = -3 is negative (entry 0)", "to_bar = 6 is below from_bar = 7 (entry 0)",
                                       "world = 0 ")):
            assert named in ln, ln
        rules = [ln[len("rule: "):] for ln in lines if ln.startswith("rule: ")]
        assert rules[0] == ""
        # ids 7, 9, 7: the first row (100 bars) answers for id 7; (9, 2, 40, 90) and (7, 0, 99, 100) are empty at T = 64
        assert next(ln for ln in lines if ln.startswith("resolved: ")) == "resolved: 2 0 64 74 2 100"
        assert rules[1] == "unknown symbol id 8 (entry 0)"
        assert rules[2] == "param 3 outside [0, 3) (entry 1)"
        assert rules[3] == "no dataset loaded"
        assert re.search(r"above 2\^30", rules[4]) and "1073741825" in rules[4]
        assert rules[5] == ""
