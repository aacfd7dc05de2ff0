"""Net of costs, the parts that need no GPU (docs/costs_spec.md): bt_costs_host, bt_costs_agg_host
and bt_costs_merge against the Python-int reference of costs_ref.py on every lane of the random
cases, the ragged rows and limit family A; the identities that tie the record to the oracle's
summaries and to the trade statistics; proof from the references alone that the cases and levels
reach the shapes the kernel's accounting can get wrong; every refusal; the record layouts
(tests/costs_abi_host.c); the chunk planner (plan_costs through tests/plan/costs_plan_driver.cpp);
and planner and host code as a stand-alone program under AddressSanitizer and UBSan
(tests/asan/costs_driver.cpp)."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import dbx_amd as D
from dbx_amd import engine as E
import costs_ref as R
import random_cases as RC
import tradestats_ref as T
from helpers import CSRC, SANITIZE, SANITIZE_ENV, assert_staging_layout, build_plan_driver, run_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = range(8)
LEVELS = R.LEVELS


def _host_array(lanes, curves, levels):
    S, P = len(lanes), len(lanes[0])
    got = np.zeros((S, P, len(levels)), D.COST_DTYPE)
    for s in range(S):
        for p in range(P):
            got[s, p] = D.costs_host(lanes[s][p], curves[s][p], levels)
    return got


# ------------------------------------------------------------ (a) the host code to the reference
@pytest.mark.parametrize("strategy", RC.STRATEGIES)
def test_host_equals_the_reference_on_every_lane_of_the_random_cases(strategy):
    traded = 0
    for seed in SEEDS:
        r = RC.lane_refs(strategy, seed)
        recs, agg = R.random_refs(strategy, seed)
        where = f"{strategy} seed {seed}"
        S, P, _ = recs.shape
        got = _host_array([[r.lanes[s][p][1] for p in range(P)] for s in range(S)],
                          [[r.curves[s][p][1] for p in range(P)] for s in range(S)], LEVELS)
        R.assert_same(got, recs, f"{where}: records")
        R.assert_same(D.costs_agg_host(got), agg, f"{where}: aggregate")
        for cuts in ((S // 2,), (1, 4)):   # a 2-way and a 3-way row split
            parts = [D.costs_agg_host(x) for x in np.split(got, cuts)]
            R.assert_same(D.merge_costs(parts), agg, f"{where}: merge of the row split {cuts}")
        R.assert_same(D.merge_costs([agg]), agg, f"{where}: merge of one part")
        traded += int(recs["n_trades"][:, :, 0].sum())
    assert traded >= 2_000


@pytest.mark.parametrize("strategy", RC.STRATEGIES)
def test_host_equals_the_reference_on_the_ragged_rows(strategy):
    series = T.ragged_series(strategy)
    grid = T.RAGGED_GRIDS[strategy]()
    lanes = R.case_lanes(strategy, grid, series)
    recs = R.case_series(strategy, grid, series, LEVELS, lanes)
    assert recs["n_bars"][:, 0, 0].tolist() == list(T.RAGGED)
    trades = [[np.array([(e, x, sd, 0, a, b) for e, x, sd, a, b in tr], D.TRADE_DTYPE) for tr, _ in row] for row in lanes]
    got = _host_array(trades, [[eq for _, eq in row] for row in lanes], LEVELS)
    R.assert_same(got, recs, f"{strategy}: ragged rows")
    R.assert_same(D.costs_agg_host(got), R.aggregate(recs), f"{strategy}: ragged rows, aggregate")
    # the 1-bar row: all zeros but n_bars and mdd_bar, on every level
    zero = np.zeros((), D.COST_DTYPE)
    zero["n_bars"], zero["mdd_bar"] = 1, -1
    assert all(x.tobytes() == zero.tobytes() for x in recs[0].reshape(-1))


@pytest.mark.parametrize("name", ("sma", "ema_ols", "boll"))
def test_host_equals_the_reference_on_family_a(name):
    """Prices near 2^31 at the limit level, and the whole ladder beside it."""
    levels = R.LIMIT + LEVELS
    grid, series, recs = R.family_a_refs(name, levels)
    _, _, _, rows = R.LC._a_case(name)
    got = np.zeros(recs.shape, D.COST_DTYPE)
    for s, ((c, _, _), (_, trades)) in enumerate(zip(series, rows)):
        for p in range(grid.n_params):
            got[s, p] = D.costs_host(trades[p], T.curves_from_trades(c, trades[p])[1], levels)
    R.assert_same(got, recs, f"family A {name}: host records")
    R.assert_same(D.costs_agg_host(got), R.aggregate(recs), f"family A {name}: host aggregate")
    assert (recs[:, :, 0].tobytes() == recs[:, :, len(levels) - 1].tobytes()), "the limit level twice"


# ----------------------------------------------------------------------------- (b) identities
@pytest.mark.parametrize("strategy", RC.STRATEGIES)
def test_identities_with_the_summaries_and_the_trade_statistics(strategy):
    for seed in SEEDS:
        c = RC.lane_case(strategy, seed)
        summ = RC.lane_refs(strategy, seed).summaries
        recs, agg = R.random_refs(strategy, seed)
        ts, _ = T.random_refs(strategy, seed)
        where = f"{strategy} seed {seed}"
        assert np.array_equal(recs["win_sum"] - recs["loss_sum"], recs["pnl"]), where
        free = recs[:, :, 0]                                  # the level (0, 0)
        for f in ("pnl", "mdd", "n_trades"):
            assert np.array_equal(free[f], summ[f]), f"{where}: {f}"
        for mine, theirs in (("n_win", "n_win"), ("n_loss", "n_loss"), ("win_sum", "gross_win"),
                             ("loss_sum", "gross_loss"), ("mdd_bar", "mdd_bar"), ("underwater_bars", "underwater_bars")):
            assert np.array_equal(free[mine], ts[theirs]), f"{where}: {mine}"
        assert not free["fees"].any()
        one = recs[:, :, 1]                                   # (1, 0): a fixed fee
        assert np.array_equal(one["fees"], 2 * one["n_trades"].astype(np.int64)), where
        for j in range(recs.shape[2]):
            assert np.array_equal(recs[:, :, j]["pnl"] + recs[:, :, j]["fees"], summ["pnl"]), f"{where}: level {j}"
            assert np.array_equal(recs[:, :, j]["turnover"], free["turnover"]), f"{where}: level {j}"
            assert np.array_equal(recs[:, :, j]["n_trades"], summ["n_trades"])
            assert np.array_equal(recs[:, :, j]["n_bars"], np.repeat(np.array(c.bars)[:, None], c.grid.n_params, 1))
        assert ((recs["mdd_bar"] == -1) == (recs["mdd"] == 0)).all()
        assert (agg["n_sym"] == len(c.series)).all() and not agg["pad"].any()
        assert (agg["n_profit"] <= agg["n_traded"]).all()


# ------------------------------------------------- (c) the cases reach the shapes that matter
# per strategy over seeds 0..7 and the ladder LEVELS, counted from the references alone: bars with
# two fills at lane 63 of a tile; trades that enter in one tile and exit in the next; exits at a
# price that is not the bar's close; lanes whose net mdd_bar differs from the gross one on some
# level; (lane, level)s that trade while the net peak stays 0; (trade, level)s that win gross and
# lose net; (trade, level)s with net_i = 0 at a level with a fee; lanes of 1 or 2 bars
REACH = {"sma": (27, 732, 0, 426, 1249, 1163, 31, 140), "ema_ols": (0, 349, 0, 129, 217, 1888, 0, 112),
         "boll": (0, 2324, 21872, 496, 2853, 9666, 0, 276)}


def _reach(strategy):
    two63 = cross = lvl = mddbar = nopeak = winloss = zero = short = 0
    for seed in SEEDS:
        c, r = RC.lane_case(strategy, seed), RC.lane_refs(strategy, seed)
        recs, _ = R.random_refs(strategy, seed)
        for s in range(len(c.series)):
            close = c.series[s][2]
            for p in range(c.grid.n_params):
                tr, eq = T.trade_tuples(r.lanes[s][p][1]), r.curves[s][p][1].tolist()
                fills = {}
                for e, x, _, _, _ in tr:
                    fills[e] = fills.get(e, 0) + 1
                    fills[x] = fills.get(x, 0) + 1
                two63 += sum(k == 2 and b % 64 == 63 for b, k in fills.items())
                cross += sum(e // 64 + 1 == x // 64 for e, x, _, _, _ in tr)
                lvl += sum(int(close[x]) != xpx for _, x, _, _, xpx in tr)
                mddbar += any(int(recs[s, p, j]["mdd_bar"]) != int(recs[s, p, 0]["mdd_bar"]) for j in range(1, len(LEVELS)))
                short += len(eq) in (1, 2)
                for j, lv in enumerate(LEVELS):
                    nopeak += bool(tr) and max(R.net_curve(tr, eq, lv)) <= 0
                    net = R.net_trades(tr, lv)
                    winloss += sum(sd * (b - a) > 0 and n < 0 for (_, _, sd, a, b), n in zip(tr, net))
                    zero += sum(n == 0 for n in net) if j else 0
    return two63, cross, lvl, mddbar, nopeak, winloss, zero, short


@pytest.mark.parametrize("strategy", RC.STRATEGIES)
def test_cases_and_levels_reach_the_shapes_that_matter(strategy):
    got = _reach(strategy)
    print(strategy, got)
    assert got == REACH[strategy]


def test_every_shape_is_reached_by_some_case():
    tot = [sum(REACH[s][k] for s in REACH) for k in range(8)]
    assert all(x >= 1 for x in tot), tot
    assert REACH["sma"][0] >= 1 and REACH["boll"][2] >= 1 and REACH["sma"][6] >= 1
    # s2 >= 2^64: family A at (2^20, 1000)
    # (the EMA+OLS grid trades too rarely on the doubling cycles: its sums stay below 2^64)
    for name, least in (("sma", 10), ("ema_ols", 0), ("boll", 10)):
        _, _, recs = R.family_a_refs(name)
        s2 = [R.s2_of(x) for x in recs.reshape(-1)]
        print(name, sum(x >= 2**64 for x in s2), len(s2), max(s2).bit_length())
        assert sum(x >= 2**64 for x in s2) >= least and max(s2) < 2**86
        assert (recs["s2_hi"] > 0).sum() == sum(x >= 2**64 for x in s2)
    # lanes of 1 and 2 bars: the ragged rows
    assert T.RAGGED[:2] == (1, 2)


def test_reference_on_hand_made_lanes():
    """The rules a reader would check by hand."""
    #  a long 100 -> 110 over bars 1..3, then a short 110 -> 104 entered on the same bar (a flip)
    tr = [(1, 3, 1, 100, 110), (3, 5, -1, 110, 104)]
    eq = [0, 0, 4, 10, 12, 16]
    r = R.lane_costs(tr, eq, (0, 0))
    assert (r["pnl"], r["fees"], r["mdd"], r["mdd_bar"], r["underwater_bars"], r["turnover"]) == (16, 0, 0, -1, 0, 424)
    r = R.lane_costs(tr, eq, (2, 0))
    # fees: 2 at bar 1, 4 at the flip bar 3, 2 at bar 5: N = 0, -2, 2, 4, 6, 8
    assert R.net_curve(tr, eq, (2, 0)) == [0, -2, 2, 4, 6, 8]
    assert (r["pnl"], r["fees"], r["mdd"], r["mdd_bar"], r["underwater_bars"]) == (8, 8, 2, 1, 1)
    assert (r["n_win"], r["n_loss"], r["win_sum"], r["loss_sum"]) == (2, 0, 8, 0) and r["s2"] == 4 + 16 + 4 + 4 + 4
    r = R.lane_costs(tr, eq, (3, 0))
    assert (r["n_win"], r["n_loss"], r["win_sum"]) == (1, 0, 4)     # the second trade nets 6 - 6 = 0: flat
    r = R.lane_costs(tr, eq, (0, 500))                               # 5 %: fees 5, 5 + 5, 5
    assert R.fee(110, (0, 500)) == 5 and R.fee(104, (0, 500)) == 5 and R.fee(19, (0, 500)) == 0
    assert (r["pnl"], r["fees"], r["n_win"], r["n_loss"], r["loss_sum"]) == (-4, 20, 0, 1, 4)
    assert (r["mdd"], r["mdd_bar"], r["underwater_bars"]) == (5, 1, 5)   # N = 0, -5, -1, -5, -3, -4: the net
    # peak never leaves 0, and of the two deepest drawdowns the first is mdd_bar
    got = D.costs_host(np.array([(e, x, s, 0, a, b) for e, x, s, a, b in tr], D.TRADE_DTYPE), eq,
                       [(0, 0), (2, 0), (3, 0), (0, 500)])
    want = np.array([R.as_record(R.lane_costs(tr, eq, lv)) for lv in ((0, 0), (2, 0), (3, 0), (0, 500))])
    R.assert_same(got, want, "hand-made lane")


# ----------------------------------------------------------------------------- (d) refusals
def test_refusals_name_the_value_and_leave_the_library_usable():
    tr = np.array([(0, 2, 1, 0, 100, 98)], D.TRADE_DTYPE)
    eq = np.array([0, 5, -2], np.int64)
    out = np.zeros(16, D.COST_DTYPE)
    agg = np.zeros(2, D.COST_AGG_DTYPE)
    lv = np.array([(1, 0), (0, 5)], np.int32)
    host, agg_host, merge = (E.sym(n) for n in ("bt_costs_host", "bt_costs_agg_host", "bt_costs_merge"))

    def last():
        return D.lib().bt_last_error().decode()

    def still_good():
        assert host(1, tr.ctypes.data, 3, eq.ctypes.data, 2, lv.ctypes.data, out.ctypes.data) == 0
        assert (int(out[0]["n_loss"]), int(out[0]["fees"]), int(out[0]["pnl"]), int(out[0]["mdd"])) == (1, 2, -4, 8)

    def levels(*pairs):
        a = np.array(pairs, np.int32)
        keep.append(a)
        return a.ctypes.data

    keep = []
    t, q, o, a, l2 = tr.ctypes.data, eq.ctypes.data, out.ctypes.data, agg.ctypes.data, lv.ctypes.data
    bad_side = np.array([(0, 2, 0, 0, 100, 98)], D.TRADE_DTYPE)
    big_px = np.array([(0, 2, 1, 0, 100, 1 << 32)], D.TRADE_DTYPE)
    for fn, args, named in (
        (host, (-1, t, 3, q, 2, l2, o), r"bt_costs_host: n_trades = -1 is negative"),
        (host, (1, t, 0, q, 2, l2, o), r"n_bars = 0 is below 1"),
        (host, (1, t, 3, q, 0, l2, o), r"C = 0 outside \[1, 16\]"),
        (host, (1, t, 3, q, 17, l2, o), r"C = 17 outside \[1, 16\]"),
        (host, (1, t, 3, q, 2, None, o), r"levels is NULL"),
        (host, (1, t, 3, q, 2, levels((0, 0), ((1 << 20) + 1, 0)), o), r"level 1: fixed = 1048577 outside \[0, 1048576\]"),
        (host, (1, t, 3, q, 2, levels((0, 1001), (0, 0)), o), r"level 0: bps = 1001 outside \[0, 1000\]"),
        (host, (1, t, 3, q, 2, levels((0, 0), (-1, 5)), o), r"level 1: fixed = -1 outside"),
        (host, (1, t, 3, q, 2, levels((0, -7), (0, 0)), o), r"level 0: bps = -7 outside"),
        (host, (1, t, 3, q, 2, l2, None), r"out is NULL"),
        (host, (1, t, 3, None, 2, l2, o), r"equity is NULL"),
        (host, (1, None, 3, q, 2, l2, o), r"trades is NULL with n_trades = 1"),
        (host, (1, t, 2, q, 2, l2, o), r"trade 0 runs \[0, 2\] outside the 2 bars"),
        (host, (1, bad_side.ctypes.data, 3, q, 2, l2, o), r"trade 0 has side 0"),
        (host, (1, big_px.ctypes.data, 3, q, 2, l2, o), r"trade 0 fills at 100 and 4294967296, outside \[0, 2\^32\)"),
        (agg_host, (-1, 1, 1, o, a), r"bt_costs_agg_host: S = -1 is negative"),
        (agg_host, (1, 0, 1, o, a), r"P = 0 is below 1"),
        (agg_host, (1, 1, 0, o, a), r"C = 0 outside \[1, 16\]"),
        (agg_host, (1, 1, 17, o, a), r"C = 17 outside \[1, 16\]"),
        (agg_host, (1, 1, 1, o, None), r"agg is NULL"),
        (agg_host, (1, 1, 1, None, a), r"recs is NULL with S = 1"),
        (merge, (a, 0, 1, a), r"bt_costs_merge: world = 0 is below 1"),
        (merge, (a, 1, 0, a), r"PC = 0 is below 1"),
        (merge, (None, 1, 1, a), r"in and out are required"),
    ):
        assert fn(*args) == -1
        assert re.search(named, last()), last()
        still_good()
    assert E.sym("bt_costs")(None, 2, l2, 0, None, o, None) == -1
    assert re.search(r"bt_costs: null engine", last()), last()
    assert E.sym("bt_set_costs_budget")(None, 0) == -1
    assert re.search(r"bt_set_costs_budget: null engine", last()), last()
    still_good()
    with pytest.raises(ValueError, match="S x P x C"):
        D.costs_agg_host(np.zeros((3, 2), D.COST_DTYPE))
    with pytest.raises(ValueError, match="different parameter or level counts"):
        D.merge_costs([np.zeros((2, 2), D.COST_AGG_DTYPE), np.zeros((3, 2), D.COST_AGG_DTYPE)])
    with pytest.raises(ValueError, match="integer pairs"):
        D.costs_host(tr, eq, [(1, 2, 3)])
    with pytest.raises(ValueError, match="int32"):
        D.costs_host(tr, eq, [(1 << 40, 0)])
    with pytest.raises(D.BtError, match=r"C = 0 outside \[1, 16\]"):
        D.costs_host(tr, eq, [])


# the rules of the call, in the order it checks them (costs_refusal), as the driver prints them
RULES = ("no dataset loaded", "C = 0 outside [1, 16]", "C = 17 outside [1, 16]", "levels is NULL",
         "level 1: fixed = 1048577 outside [0, 1048576]", "level 0: bps = 1001 outside [0, 1000]",
         "n = -1 outside [0, 1048576]", "n = 1048577 outside [0, 1048576]",
         "n = 3 with lanes == NULL (all-lanes mode takes n = 0)", "agg given in list mode (n = 3 lanes): it must be NULL",
         "out is required in list mode (n = 3 lanes)", "out and agg are both NULL", "", "", "levels is NULL", "",
         "P * C = 400 * 8 records of one row (281600 bytes) exceed the staging budget of 1000 bytes")
REFUSED = ("n_trades = -1 ", "n_bars = 0 ", "C = 0 ", "C = 17 ", "levels is NULL", "level 1: fixed = 1048577",
           "level 0: bps = 1001", "level 0: fixed = -1", "level 1: bps = -5", "out is NULL", "equity is NULL",
           "trades is NULL", "outside the 2 bars", "side 0", "outside [0, 2^32)", "S = -1 ", "P = 0 ", "C = 0 ",
           "agg is NULL", "recs is NULL", "world = 0 ", "PC = 0 ", "in and out")


# ------------------------------------------------------------------------------------ layout
def test_record_layouts_match_the_c99_host(tmp_path):
    """The two records' mirror (costs.py COST_RECORDS) has the header's sizes and offsets, field by
    field, and every struct a bt_costs* entry point takes is one of them (or of the engine's)."""
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    exe = str(tmp_path / "costs_abi_host")
    r = subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "costs_abi_host.c"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(subprocess.run([exe], capture_output=True, text=True, check=True).stdout)
    assert got.pop("abi_version") == 3 == D.ABI_VERSION
    assert (got.pop("costs_max"), got.pop("levels_max"), got.pop("fixed_max"), got.pop("bps_max")) == \
        (D.COSTS_MAX, D.COST_LEVELS_MAX, D.COST_FIXED_MAX, D.COST_BPS_MAX) == (1 << 20, 16, 1 << 20, 1000)
    assert list(D.COST_RECORDS) == ["bt_cost_rec", "bt_cost_agg"]
    assert D.COST_DTYPE.itemsize == 88 and D.COST_AGG_DTYPE.itemsize == 48
    for cname, dt in D.COST_RECORDS.items():
        assert got.pop(cname) == dt.itemsize, cname
        for f in dt.names:
            assert got.pop(f"{cname}.{f}") == dt.fields[f][1], f"{cname}.{f}"
    assert not got, f"fields the mirror lacks: {sorted(got)}"
    hdr = open(os.path.join(ROOT, "include", "bt.h")).read()
    assert "#define BT_ABI_VERSION 3" in hdr
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    protos = re.findall(r"\b(bt_costs[a-z0-9_]*)\s*\(([^()]*)\)\s*;", hdr)
    assert sorted(n for n, _ in protos) == ["bt_costs", "bt_costs_agg_host", "bt_costs_host", "bt_costs_merge"]
    taken = {t for _, args in protos for t in re.findall(r"\b(bt_\w+)\s*\*", args)}
    assert taken - {"bt_engine"} <= set(D.COST_RECORDS) | set(E.RECORDS) and set(D.COST_RECORDS) <= taken
    # engine.py names none of the entry points (tests/test_abi_cpu.py reads it for the calls it checks)
    binding = open(E.__file__).read()
    for name in ("bt_costs", "bt_set_costs_budget", "bt_costs_host", "bt_costs_agg_host", "bt_costs_merge"):
        assert not re.search(rf"\b{name}\b", binding), name
        assert E.sym(name) is not None


def test_derived_figures_are_zero_where_the_denominator_is():
    tr = [(1, 3, 1, 100, 110), (3, 5, -1, 110, 104)]
    eq = [0, 0, 4, 10, 12, 16]
    levels = [(0, 0), (2, 0), (0, 500)]
    recs = np.zeros((1, 2, 3), D.COST_DTYPE)
    recs[0, 0] = [R.as_record(R.lane_costs(tr, eq, lv)) for lv in levels]
    recs[0, 1] = [R.as_record(R.lane_costs([], [0] * 6, lv)) for lv in levels]
    cs = D.Costs(D.costs.as_levels(levels), recs, D.costs_agg_host(recs))
    assert cs.win_rate().tolist() == [[[1.0, 1.0, 0.0], [0.0, 0.0, 0.0]]]
    assert cs.profit_factor().tolist() == [[[0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]]     # no losses, or no wins
    assert cs.breakeven_fixed().tolist() == [[[4.0, 4.0, 4.0], [0.0, 0.0, 0.0]]]   # 16 / (2 * 2)
    assert np.allclose(cs.breakeven_bps(), [[[16e4 / 424] * 3, [0.0] * 3]], rtol=1e-15)
    assert cs.s2.tolist() == [[[16 + 36 + 4 + 16, 4 + 16 + 4 + 4 + 4, 25 + 16 + 16 + 4 + 1], [0, 0, 0]]]
    assert all(type(x) is int for x in cs.s2.reshape(-1))
    m, v = 8 / 6, 32 / 6 - (8 / 6) ** 2
    assert cs.net_sharpe(252)[0, 0, 1] == (m / np.sqrt(v)) * np.sqrt(252.0) and cs.net_sharpe()[0, 1].tolist() == [0.0] * 3
    assert cs.survivors().tolist() == [[1.0, 1.0, 0.0], [0.0, 0.0, 0.0]]
    assert cs.rank(0).tolist() == [0, 1] and cs.rank(2).tolist() == [1, 0] and cs.rank(2, 1).tolist() == [1]
    tie = D.Costs(cs.levels, None, np.zeros((4, 3), D.COST_AGG_DTYPE))
    assert tie.rank(1).tolist() == [0, 1, 2, 3]                                     # ties to the lower index
    with pytest.raises(ValueError, match="not asked for"):
        tie.win_rate()
    with pytest.raises(ValueError, match="not asked for"):
        D.Costs(cs.levels, recs, None).survivors()
    with pytest.raises(ValueError, match=r"level 3 outside \[0, 3\)"):
        cs.rank(3)


# ------------------------------------------------------------------------------ (e) planner
@pytest.fixture(scope="module")
def plan():
    exe = build_plan_driver("costs_plan_driver")

    def run(units, P, C, list_mode=0, cus=256, budget=0):
        return run_driver(exe, units, P, C, int(list_mode), cus, budget)
    return run


BUDGET = 256 << 20
# name: (units, P, C, list mode, budget_req)
PLAN_SHAPES = {
    "config2_c8": (5000, 400, 8, 0, 0), "config2_c1": (5000, 400, 1, 0, 0), "config3_c16": (500, 64, 16, 0, 0),
    "one": (1, 1, 1, 0, 0), "one_row_chunks": (6, 36, 5, 0, R.rows_budget(36, 5, 1)),
    "small_budget": (9, 12, 3, 0, 40000), "list_max": (1 << 20, 400, 2, 1, 0), "list_one": (1, 400, 16, 1, 0),
    "list_small_budget": (1000, 7, 5, 1, 20000),
}


@pytest.mark.parametrize("name", list(PLAN_SHAPES))
def test_plan_costs_covers_every_unit_once_within_the_budget(plan, name):
    units, P, C, lst, req = PLAN_SHAPES[name]
    pl = plan(units, P, C, lst, 256, req)
    assert pl == plan(units, P, C, lst, 256, req), "the plan is a function of its arguments"
    assert pl["budget"] == BUDGET and pl["rec_bytes"] == 88 and pl["agg_bytes"] == 48 and pl["lane_bytes"] == 16
    assert pl["list"] == lst and pl["C"] == C
    budget = req or BUDGET
    per = pl["per_chunk"]
    assert 1 <= per <= units
    if lst:
        assert pl["unit_bytes"] == 16 + C * 88
        regions = [(pl["o_lanes"], per * 16), (pl["o_rec"], per * C * 88)]
        assert pl["o_lanes"] == 0 and pl["waves"] == per and per <= 1 << 30
    else:
        assert pl["unit_bytes"] == P * C * 88
        regions = [(pl["o_agg"], P * C * 48), (pl["o_rec"], per * P * C * 88)]
        assert pl["o_agg"] == 0 and pl["waves"] == per * P and per * P <= 1 << 30
    assert_staging_layout(regions, pl["staging_bytes"], name)
    assert pl["staging_bytes"] <= budget
    # as many units as fit: one more would pass the budget (or there is no more)
    assert per == units or pl["staging_bytes"] + pl["unit_bytes"] > budget
    assert pl["chunks"] == -(-units // per)
    rows = pl["units"]
    assert rows[0][0] == 0 and rows[-1][1] == units
    assert all(a[1] == b[0] for a, b in zip(rows[:-1], rows[1:]) if pl["chunks"] <= 8), "chunks are contiguous"
    assert all(0 < r1 - r0 <= per for r0, r1 in rows)
    # the reduction: every (parameter, level) has a thread, and the slices hold every row of a chunk
    assert pl["agg_block"] % 64 == 0 and 64 <= pl["agg_block"] <= 256
    assert pl["agg_pblocks"] * pl["agg_block"] >= P * C > (pl["agg_pblocks"] - 1) * pl["agg_block"]
    assert (pl["slice_rows"], pl["max_slices"]) == (64, 64) and 1 <= pl["agg_slices"] <= 64
    assert pl["agg_slices"] == min(-(-per // 64), 64)


def test_plan_costs_on_the_shapes_of_the_call(plan):
    c8 = plan(5000, 400, 8)       # 1.41 GB of records: six chunks under the default budget
    assert c8["per_chunk"] == (BUDGET - 400 * 8 * 48 - 256) // (400 * 8 * 88) == 952 and c8["chunks"] == 6
    assert c8["agg_slices"] == 15 and c8["agg_block"] == 256 and c8["agg_pblocks"] == 13
    c1 = plan(5000, 400, 1)
    assert c1["chunks"] == 1 and c1["per_chunk"] == 5000 and c1["staging_bytes"] < BUDGET
    assert plan(6, 36, 5, 0, 256, R.rows_budget(36, 5, 1))["chunks"] == 6      # exactly one row per chunk
    assert plan(6, 36, 5, 0, 256, R.rows_budget(36, 5, 2))["chunks"] == 3
    # the many-row tests of the GPU file: family A x 205 rows under the two budgets of the trade statistics
    for name, P in (("sma", 9), ("boll", 24)):
        for rows, (chunks, slices) in ((0, (1, 4)), (100, (3, 2)), (200, (2, 4))):
            pl = plan(T.A_ROWS, P, 1, 0, 256, R.rows_budget(P, 1, rows) if rows else 0)
            assert (pl["per_chunk"], pl["chunks"], pl["agg_slices"]) == (rows or T.A_ROWS, chunks, slices), (name, rows)
    # one unit that cannot fit: the plan says so with per_chunk 0 and the call is refused
    for args in ((3, 400, 8, 0, 256, 400 * 8 * 88), (3, 1 << 20, 16, 0, 256, 100 << 20), (5, 7, 16, 1, 256, 600)):
        pl = plan(*args)
        assert pl["per_chunk"] == 0 and pl["chunks"] == 0 and pl["staging_bytes"] == 0


def test_plan_driver_under_asan_and_ubsan():
    exe = build_plan_driver("costs_plan_driver", sanitize=True)
    for name in ("one_row_chunks", "list_small_budget"):
        units, P, C, lst, req = PLAN_SHAPES[name]
        assert run_driver(exe, units, P, C, lst, 256, req, sanitized=True) == \
            run_driver(build_plan_driver("costs_plan_driver"), units, P, C, lst, 256, req)


# ---------------------------------------------------------------------- (f) under the sanitizers
def test_planner_and_host_code_under_asan_and_ubsan(tmp_path):
    """tests/asan/costs_driver.cpp with csrc/costs.cpp and csrc/plan.cpp: a program of its own, built
    with the sanitizers and run directly."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc missing")
    exe = str(tmp_path / "costs_asan")
    r = subprocess.run([hipcc, "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", *SANITIZE, "-x", "hip",
                        "--cuda-host-only", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "asan", "costs_driver.cpp"), os.path.join(CSRC, "costs.cpp"),
                        os.path.join(CSRC, "plan.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    traded = 0
    lv = np.array(LEVELS, np.int32)
    for strategy, seed in (("sma", 0), ("ema_ols", 1), ("boll", 2)):
        rf = RC.lane_refs(strategy, seed)
        recs, agg = R.random_refs(strategy, seed)
        S, P, C = recs.shape
        fin, fout = str(tmp_path / f"in_{strategy}"), str(tmp_path / f"out_{strategy}")
        with open(fin, "wb") as f:
            f.write(np.array([S, P, C], np.int32).tobytes() + lv.tobytes())
            for s in range(S):
                for p in range(P):
                    tr, eq = rf.lanes[s][p][1], rf.curves[s][p][1]
                    tr = np.zeros(0, D.TRADE_DTYPE) if tr is None else np.ascontiguousarray(tr, D.TRADE_DTYPE)
                    f.write(np.array([len(tr), len(eq)], np.int32).tobytes() + tr.tobytes()
                            + np.ascontiguousarray(eq, np.int64).tobytes())
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, env=SANITIZE_ENV, timeout=120)
        assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
        raw = open(fout, "rb").read()
        nr, na = S * P * C * 88, P * C * 48
        assert len(raw) == nr + 2 * na
        R.assert_same(np.frombuffer(raw[:nr], D.COST_DTYPE).reshape(S, P, C), recs, f"{strategy}: records")
        R.assert_same(np.frombuffer(raw[nr:nr + na], D.COST_AGG_DTYPE).reshape(P, C), agg, f"{strategy}: aggregate")
        R.assert_same(np.frombuffer(raw[nr + na:], D.COST_AGG_DTYPE).reshape(P, C), agg, f"{strategy}: merged halves")
        traded += int(recs["n_trades"][:, :, 0].sum())
        lines = r.stdout.splitlines()
        assert lines[-1] == f"ok {S} {P} {C}"
        refused = [ln for ln in lines if ln.startswith("refused: ")]
        assert len(refused) == len(REFUSED)
        for ln, named in zip(refused, REFUSED):
            assert named in ln, (ln, named)
        assert [ln[len("rule: "):] for ln in lines if ln.startswith("rule: ")] == list(RULES)
        plans = [tuple(int(x) for x in ln.split()[1:]) for ln in lines if ln.startswith("plan: ")]
        assert len(plans) == 3 and plans[0][:2] == (S, 1) and plans[1][:2] == (1, S) and plans[2] == (0, 0, 1, 0)
    assert traded >= 500
