"""Per-lane trade statistics, the parts that need no GPU (docs/tradestats_spec.md):
bt_trade_stats_host, bt_tstats_agg_host and bt_tstats_merge against the Python-int reference of
tradestats_ref.py on every lane of the random cases, the identities that tie the record to the
oracle's summaries, proof from the references alone that the cases reach the shapes the kernel's
accounting can get wrong, the refusals, the record layouts, the chunk planner (plan_tstats through
tests/plan/tstats_plan_driver.cpp) and the host code as a stand-alone program under
AddressSanitizer and UBSan (tests/asan/tstats_driver.cpp)."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import dbx_amd as D
from dbx_amd import engine as E
import random_cases as RC
import tradestats_ref as T
from helpers import assert_staging_layout, build_plan_driver, run_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed-backtesting-exploration_amd", "csrc")
SEEDS = range(8)


def _host_matrix(c, r):
    S, P = len(c.series), c.grid.n_params
    got = np.zeros((S, P), D.TSTATS_DTYPE)
    for s in range(S):
        for p in range(P):
            got[s, p] = D.trade_stats_host(r.lanes[s][p][1], r.curves[s][p][1])
    return got


# ------------------------------------------------------------ (a) the host code to the reference
@pytest.mark.parametrize("strategy", RC.STRATEGIES)
def test_host_equals_the_reference_on_every_lane_of_the_random_cases(strategy):
    traded = 0
    for seed in SEEDS:
        c, r = RC.lane_case(strategy, seed), RC.lane_refs(strategy, seed)
        recs, agg = T.random_refs(strategy, seed)
        where = f"{strategy} seed {seed}"
        got = _host_matrix(c, r)
        T.assert_same(got, recs, f"{where}: records")
        T.assert_same(D.trade_stats_agg_host(got), agg, f"{where}: aggregate")
        S = len(c.series)
        for cuts in ((S // 2,), (1, 4)):   # a 2-way and a 3-way row split
            parts = [D.trade_stats_agg_host(x) for x in np.split(got, cuts)]
            T.assert_same(D.merge_trade_stats(parts), agg, f"{where}: merge of the row split {cuts}")
        T.assert_same(D.merge_trade_stats([agg]), agg, f"{where}: merge of one part")
        traded += int(recs["n_trades"].sum())
    assert traded >= 2_000


@pytest.mark.parametrize("strategy", RC.STRATEGIES)
def test_identities_with_the_oracle_summaries(strategy):
    """n_trades, mdd and hash are the lane's bt_summary; gross_win - gross_loss its pnl; hold_sum
    its exposure."""
    for seed in SEEDS:
        c = RC.lane_case(strategy, seed)
        summ = RC.lane_refs(strategy, seed).summaries
        recs, _ = T.random_refs(strategy, seed)
        for f in ("n_trades", "mdd", "hash"):
            assert np.array_equal(recs[f], summ[f]), f"{strategy} seed {seed}: {f}"
        assert np.array_equal(recs["gross_win"] - recs["gross_loss"], summ["pnl"]), f"{strategy} seed {seed}: pnl"
        assert np.array_equal(recs["hold_sum"], summ["exposure"]), f"{strategy} seed {seed}: exposure"
        assert np.array_equal(recs["n_bars"], np.repeat(np.array(c.bars)[:, None], c.grid.n_params, 1))
        assert not recs["status"].any()
        flat = recs["n_trades"] - recs["n_win"] - recs["n_loss"]
        assert (flat >= 0).all() and (recs["n_long_win"] <= np.minimum(recs["n_long"], recs["n_win"])).all()
        none = recs["mdd"] == 0
        assert ((recs["mdd_bar"] == -1) == none).all() and ((recs["peak_bar"] == -1) == none).all()
        assert (recs["peak_bar"][~none] < recs["mdd_bar"][~none]).all()
        assert (recs["max_underwater"] <= recs["underwater_bars"]).all()


# ------------------------------------------------- (b) the cases reach the shapes that matter
# per strategy over seeds 0..7, counted from the references alone: trades held across a 64-bar
# tile edge, exits on a tile's first and last bar, lanes without a trade, lanes whose longest
# under-water run exceeds a tile, lanes whose mdd is attained at more than one bar, the longest
# loss streak, flat trades, and flat trades that directly follow a win or a loss
SHAPES = {"sma": (1192, 76, 89, 506, 219, 130, 21, 336, 145), "ema_ols": (480, 31, 46, 633, 102, 2, 4, 3, 0),
          "boll": (2386, 564, 422, 648, 638, 505, 103, 0, 0)}


@pytest.mark.parametrize("strategy", RC.STRATEGIES)
def test_random_cases_reach_the_shapes_that_matter(strategy):
    cross = first = last = none = long_uw = multi = streak = flat = breaks = 0
    for seed in SEEDS:
        c, r = RC.lane_case(strategy, seed), RC.lane_refs(strategy, seed)
        recs, _ = T.random_refs(strategy, seed)
        for s in range(len(c.series)):
            for p in range(c.grid.n_params):
                tr = T.trade_tuples(r.lanes[s][p][1])
                eq = r.curves[s][p][1]
                cross += sum(e // 64 != x // 64 for e, x, _, _, _ in tr)
                first += sum(x % 64 == 0 for _, x, _, _, _ in tr)
                last += sum(x % 64 == 63 for _, x, _, _, _ in tr)
                none += not tr
                long_uw += int(recs[s, p]["max_underwater"]) > 64
                dd = np.maximum.accumulate(np.maximum(eq, 0)) - eq
                multi += bool(dd.max() > 0 and (dd == dd.max()).sum() > 1)
                streak = max(streak, int(recs[s, p]["max_loss_streak"]))
                pnl = [side * (xpx - epx) for _, _, side, epx, xpx in tr]
                flat += sum(x == 0 for x in pnl)
                breaks += sum(pnl[i] == 0 and pnl[i - 1] != 0 for i in range(1, len(pnl)))
    assert (cross, first, last, none, long_uw, multi, streak, flat, breaks) == SHAPES[strategy]


def test_family_a_bollinger_passes_int64_in_sq():
    """The doubling cycles: at least 100 of the Bollinger case's 432 lanes have a sum of squared
    pnl of 2^64 or more, the largest below 2^68."""
    _, _, recs = T.family_a_refs("boll")
    sq = [T.sq_of(x) for x in recs.reshape(-1)]
    assert len(sq) == 432
    assert sum(x >= 2**64 for x in sq) >= 100 and 2**64 <= max(sq) < 2**68
    assert (recs["sq_hi"] > 0).sum() == sum(x >= 2**64 for x in sq)
    got = np.zeros(recs.shape, D.TSTATS_DTYPE)
    strategy, grid, series, rows = T.LC._a_case("boll")
    for s, ((c, _, _), (_, trades)) in enumerate(zip(series, rows)):
        for p in range(grid.n_params):
            got[s, p] = D.trade_stats_host(trades[p], T.curves_from_trades(c, trades[p])[1])
    T.assert_same(got, recs, "family A, Bollinger: host records")
    T.assert_same(D.trade_stats_agg_host(got), T.aggregate(recs), "family A, Bollinger: host aggregate")


def test_the_vectorised_reference_is_the_loop_s():
    """lane_stats_fast (numpy, the reference of the rows of 2^22 bars) against lane_stats on every
    lane of family A and of the default random cases, field for field."""
    lanes = traded = 0
    for name in ("sma", "ema_ols", "boll"):
        _, grid, series, rows = T.LC._a_case(name)
        _, _, recs = T.family_a_refs(name)
        fast = np.zeros(recs.shape, D.TSTATS_DTYPE)
        for s, ((c, _, _), (_, trades)) in enumerate(zip(series, rows)):
            for p in range(grid.n_params):
                fast[s, p] = T.as_record(T.lane_stats_fast(trades[p], T.curves_from_trades(c, trades[p])[1]))
        T.assert_same(fast, recs, f"family A {name}")
        lanes += recs.size
    for strategy in RC.STRATEGIES:
        for seed in SEEDS:
            r = RC.lane_refs(strategy, seed)
            recs, _ = T.random_refs(strategy, seed)
            fast = np.zeros(recs.shape, D.TSTATS_DTYPE)
            for s in range(recs.shape[0]):
                for p in range(recs.shape[1]):
                    fast[s, p] = T.as_record(T.lane_stats_fast(r.lanes[s][p][1], r.curves[s][p][1]))
            T.assert_same(fast, recs, f"{strategy} seed {seed}")
            lanes += recs.size
            traded += int((recs["n_trades"] > 0).sum())
    assert lanes >= 81 + 36 + 432 + 24 * 6 and traded >= 1000
    r = T.lane_stats_fast(None, [0, 3, 1])      # no trade: the loop's record too
    assert r == T.lane_stats([], [0, 3, 1])
    assert T.longest_run_fast([]) == 0 and T.longest_run_fast([1, 1, 0, 1, 1, 1]) == 3 == T.longest_run([1, 1, 0, 1, 1, 1])


def test_reference_on_hand_made_lanes():
    """The rules a reader would check by hand: the tie is not a new peak and ends the run under
    water, of two equal deepest drawdowns the first wins, a flat trade ends both streaks."""
    #     t: 0  1  2  3  4  5  6  7  8
    eq = [0, 4, 1, 4, 0, 4, 9, 5, 9]
    r = T.lane_stats([], eq)
    assert (r["mdd"], r["mdd_bar"], r["peak_bar"]) == (4, 4, 1)
    assert (r["underwater_bars"], r["max_underwater"]) == (3, 1)
    r = T.lane_stats([], [0, -3, -1, -3, 0, 2, -1])
    assert (r["mdd"], r["mdd_bar"], r["peak_bar"], r["underwater_bars"], r["max_underwater"]) == (3, 1, 0, 4, 3)
    r = T.lane_stats([], [0, 1, 2, 2, 3])
    assert (r["mdd"], r["mdd_bar"], r["peak_bar"], r["underwater_bars"], r["max_underwater"]) == (0, -1, -1, 0, 0)
    # pnl: -1, -2, 0, -3, +5, +1, 0, +2  (long, short, long, ...)
    px = [(10, 9), (10, 12), (7, 7), (10, 13), (10, 15), (4, 3), (3, 3), (8, 6)]
    tr = [(2 * i, 2 * i + 1 + (i == 3), 1 if i % 2 == 0 else -1, a, b) for i, (a, b) in enumerate(px)]
    r = T.lane_stats(tr, [0] * 20)
    assert (r["n_trades"], r["n_win"], r["n_loss"], r["n_long"], r["n_long_win"]) == (8, 3, 3, 4, 1)
    assert (r["max_win_streak"], r["max_loss_streak"]) == (2, 2)
    assert (r["gross_win"], r["gross_loss"], r["max_win"], r["max_loss"], r["sq"]) == (8, 6, 5, 3, 44)
    assert (r["hold_sum"], r["hold_win"], r["hold_max"]) == (9, 3, 2)
    got = D.trade_stats_host(np.array([(e, x, s, 0, a, b) for e, x, s, a, b in tr], D.TRADE_DTYPE), [0] * 20)
    T.assert_same(np.array([got]), np.array([T.as_record(r)]), "hand-made trades")


# ----------------------------------------------------------------------------- (c) refusals
def test_refusals_name_the_value_and_leave_the_library_usable():
    tr = np.array([(0, 2, 1, 0, 100, 98)], D.TRADE_DTYPE)
    eq = np.array([0, 5, -2], np.int64)
    out = np.zeros(1, D.TSTATS_DTYPE)
    agg = np.zeros(2, D.TSTATS_AGG_DTYPE)
    host, agg_host, merge = (E.sym(n) for n in ("bt_trade_stats_host", "bt_tstats_agg_host", "bt_tstats_merge"))

    def last():
        return D.lib().bt_last_error().decode()

    def still_good():
        assert host(1, tr.ctypes.data, 3, eq.ctypes.data, out.ctypes.data) == 0
        assert (int(out[0]["n_loss"]), int(out[0]["gross_loss"]), int(out[0]["mdd"]), int(out[0]["mdd_bar"])) == (1, 2, 7, 2)

    t, q, o, a = tr.ctypes.data, eq.ctypes.data, out.ctypes.data, agg.ctypes.data
    bad_side = np.array([(0, 2, 0, 0, 100, 98)], D.TRADE_DTYPE)
    for fn, args, named in (
        (host, (-1, t, 3, q, o), r"bt_trade_stats_host: n_trades = -1 is negative"),
        (host, (1, t, 0, q, o), r"n_bars = 0 is below 1"),
        (host, (1, t, 3, q, None), r"out is NULL"),
        (host, (1, t, 3, None, o), r"equity is NULL"),
        (host, (1, None, 3, q, o), r"trades is NULL with n_trades = 1"),
        (host, (1, t, 2, q, o), r"trade 0 runs \[0, 2\] outside the 2 bars"),
        (host, (1, bad_side.ctypes.data, 3, q, o), r"trade 0 has side 0"),
        (agg_host, (-1, 1, o, a), r"bt_tstats_agg_host: S = -1 is negative"),
        (agg_host, (1, 0, o, a), r"P = 0 is below 1"),
        (agg_host, (1, 1, o, None), r"agg is NULL"),
        (agg_host, (1, 1, None, a), r"recs is NULL with S = 1"),
        (merge, (a, 0, 1, a), r"bt_tstats_merge: world = 0 is below 1"),
        (merge, (a, 1, 0, a), r"P = 0 is below 1"),
        (merge, (None, 1, 1, a), r"in and out are required"),
    ):
        assert fn(*args) == -1
        assert re.search(named, last()), last()
        still_good()
    assert E.sym("bt_trade_stats")(None, 0, None, o, None) == -1
    assert re.search(r"bt_trade_stats: null engine", last()), last()
    assert E.sym("bt_set_tstats_budget")(None, 0) == -1
    assert re.search(r"bt_set_tstats_budget: null engine", last()), last()
    still_good()
    with pytest.raises(ValueError, match="S x P"):
        D.trade_stats_agg_host(np.zeros(3, D.TSTATS_DTYPE))
    with pytest.raises(ValueError, match="parameter counts"):
        D.merge_trade_stats([np.zeros(2, D.TSTATS_AGG_DTYPE), np.zeros(3, D.TSTATS_AGG_DTYPE)])


def test_derived_figures_are_zero_where_the_denominator_is():
    recs = np.zeros((1, 3), D.TSTATS_DTYPE)
    recs[0, 1] = T.as_record(T.lane_stats([(0, 1, 1, 10, 14), (2, 4, 1, 10, 8), (5, 6, -1, 9, 3)], [0] * 8))
    recs[0, 2] = T.as_record(T.lane_stats([(0, 3, 1, 10, 14)], [0] * 8))
    ts = D.TradeStats(recs, D.trade_stats_agg_host(recs))
    assert ts.win_rate().tolist() == [[0.0, 2 / 3, 1.0]] and ts.profit_factor().tolist() == [[0.0, 5.0, 0.0]]
    assert ts.expectancy().tolist() == [[0.0, 8 / 3, 4.0]] and ts.avg_win().tolist() == [[0.0, 5.0, 4.0]]
    assert ts.avg_loss().tolist() == [[0.0, 2.0, 0.0]] and ts.payoff().tolist() == [[0.0, 2.5, 0.0]]
    assert ts.avg_hold().tolist() == [[0.0, 4 / 3, 3.0]]
    assert ts.sq.tolist() == [[0, 56, 16]] and all(type(x) is int for x in ts.sq.reshape(-1))
    std = np.sqrt(56 / 3 - (8 / 3) ** 2)
    assert np.allclose(ts.trade_std(), [[0.0, std, 0.0]], rtol=1e-15)
    assert np.allclose(ts.t_stat(), [[0.0, (8 / 3) * np.sqrt(3) / std, 0.0]], rtol=1e-15)
    assert ts.win_rate(params=True).tolist() == [0.0, 2 / 3, 1.0] and ts.params_sq.tolist() == [0, 56, 16]
    with pytest.raises(ValueError, match="not asked for"):
        D.TradeStats(recs, None).win_rate(params=True)


# ------------------------------------------------------------------------------------ layout
def test_record_layouts(tmp_path):
    assert D.TSTATS_DTYPE.itemsize == 128 and D.TSTATS_AGG_DTYPE.itemsize == 136 and D.TSTATS_MAX == 1 << 20
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "layout.c"
    lines = ['    printf("{\\"bt_tstats\\": %d, \\"bt_tstats_agg\\": %d, \\"max\\": %d", (int)sizeof(bt_tstats), '
             '(int)sizeof(bt_tstats_agg), (int)BT_TSTATS_MAX);\n']
    for st, dt in (("bt_tstats", D.TSTATS_DTYPE), ("bt_tstats_agg", D.TSTATS_AGG_DTYPE)):
        lines += [f'    printf(", \\"{st}.{f}\\": %d", (int)offsetof({st}, {f}));\n' for f in dt.names]
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bt.h"\nint main(void) {\n' + "".join(lines) +
                   '    printf("}\\n");\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    r = subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(subprocess.run([exe], capture_output=True, text=True, check=True).stdout)
    assert got.pop("bt_tstats") == 128 and got.pop("bt_tstats_agg") == 136 and got.pop("max") == D.TSTATS_MAX
    want = {f"bt_tstats.{f}": D.TSTATS_DTYPE.fields[f][1] for f in D.TSTATS_DTYPE.names}
    want.update({f"bt_tstats_agg.{f}": D.TSTATS_AGG_DTYPE.fields[f][1] for f in D.TSTATS_AGG_DTYPE.names})
    assert got == want


# ------------------------------------------------------------------------------ (d) planner
@pytest.fixture(scope="module")
def plan():
    exe = build_plan_driver("tstats_plan_driver")

    def run(units, P, list_mode=0, cus=256, budget=0):
        return run_driver(exe, units, P, int(list_mode), cus, budget)
    return run


BUDGET = 256 << 20
# name: (units, P, list mode, budget_req)
PLAN_SHAPES = {
    "config2": (5000, 400, 0, 0), "config2_two_shards": (10000, 400, 0, 0), "config3": (500, 64, 0, 0),
    "one": (1, 1, 0, 0), "many_params": (3, 1 << 19, 0, 0), "one_row_chunks": (6, 36, 0, 36 * 136 + 36 * 128 + 600),
    "small_budget": (9, 12, 0, 40000), "list_max": (1 << 20, 400, 1, 0), "list_one": (1, 400, 1, 0),
    "list_small_budget": (1000, 7, 1, 20000), "list_more_than_fit": (1 << 20, 400, 1, 64 << 20),
}


@pytest.mark.parametrize("name", list(PLAN_SHAPES))
def test_plan_tstats_covers_every_unit_once_within_the_budget(plan, name):
    units, P, lst, req = PLAN_SHAPES[name]
    pl = plan(units, P, lst, 256, req)
    assert pl == plan(units, P, lst, 256, req), "the plan is a function of its arguments"
    assert pl["budget"] == BUDGET and pl["rec_bytes"] == 128 and pl["agg_bytes"] == 136 and pl["lane_bytes"] == 16
    assert pl["list"] == lst
    budget = req or BUDGET
    per = pl["per_chunk"]
    assert 1 <= per <= units
    if lst:
        assert pl["unit_bytes"] == 16 + 128
        regions = [(pl["o_lanes"], per * 16), (pl["o_rec"], per * 128)]
        assert pl["o_lanes"] == 0 and pl["waves"] == per and per <= 1 << 30
    else:
        assert pl["unit_bytes"] == P * 128
        regions = [(pl["o_agg"], P * 136), (pl["o_rec"], per * P * 128)]
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
    # the reduction: every parameter has a thread, and the slices hold every row of a chunk
    assert pl["agg_block"] % 64 == 0 and 64 <= pl["agg_block"] <= 256
    assert pl["agg_pblocks"] * pl["agg_block"] >= P > (pl["agg_pblocks"] - 1) * pl["agg_block"]
    assert (pl["slice_rows"], pl["max_slices"]) == (64, 64) and 1 <= pl["agg_slices"] <= 64
    assert pl["agg_slices"] == min(-(-per // 64), 64)


def test_plan_tstats_on_the_shapes_of_the_issue(plan):
    c2 = plan(5000, 400)
    assert c2["chunks"] == 1 and c2["per_chunk"] == 5000 and c2["staging_bytes"] < BUDGET and c2["fill"] > 200
    two = plan(10000, 400)
    assert two["chunks"] == 2 and two["per_chunk"] == (BUDGET - 54528 - 256) // (400 * 128)
    assert plan(6, 36, 0, 256, 36 * 136 + 36 * 128 + 600)["chunks"] == 6      # exactly one row per chunk
    full = plan(1 << 20, 400, 1)
    assert full["chunks"] == 1 and full["staging_bytes"] <= (1 << 20) * 144 + 512
    assert plan(1 << 20, 400, 1, 256, 64 << 20)["chunks"] == 3
    # one row that cannot fit: the plan says so with per_chunk 0 and the call is refused
    for args in ((3, 400, 0, 256, 400 * 128), (3, 1 << 20, 0, 256, 100 << 20), (5, 7, 1, 256, 600)):
        pl = plan(*args)
        assert pl["per_chunk"] == 0 and pl["chunks"] == 0 and pl["staging_bytes"] == 0


# chunk rows (0: the default budget) -> (chunks, agg_slices, the slices' row ranges chunk by chunk)
MANY_ROWS_GEOMETRY = {
    0: (1, 4, [[(0, 52), (52, 104), (104, 156), (156, 205)]]),
    100: (3, 2, [[(0, 50), (50, 100)], [(0, 50), (50, 100)], [(0, 3), (3, 5)]]),
    # the short last chunk: ceil(5 / 4) = 2 rows a slice, the fourth begins at row 6 of 5
    200: (2, 4, [[(0, 50), (50, 100), (100, 150), (150, 200)], [(0, 2), (2, 4), (4, 5), (6, 5)]]),
}
# parameters of family A x 205 rows whose slices' low words add up to 2^64 or more, under every one
# of the three budgets, and the largest such sum in units of 2^64 (rounded down)
MANY_ROWS_CARRY = {"sma": (7, 2), "boll": (15, 3)}


@pytest.mark.parametrize("name", ("sma", "boll"))
def test_many_rows_reach_several_slices_an_empty_slice_and_the_carry(plan, name):
    """test_gpu_tradestats.test_family_a_many_rows_in_slices_and_chunks: the plan of each budget,
    the row range of every slice of every chunk, and that the atomic adds into sq_lo wrap."""
    grid, series, recs = T.family_a_many_rows(name)
    R, P = recs.shape
    assert R == T.A_ROWS == len(series) == 205 and tuple(MANY_ROWS_GEOMETRY) == (0,) + T.A_CHUNK_ROWS
    for rows, (chunks, slices, ranges) in MANY_ROWS_GEOMETRY.items():
        pl = plan(R, P, 0, 256, T.rows_budget(P, rows) if rows else 0)
        assert (pl["per_chunk"], pl["chunks"], pl["agg_slices"]) == (rows or R, chunks, slices) and slices >= 2
        units = [tuple(u) for u in pl["units"]]
        assert len(units) == chunks and [T.agg_slice_rows(r1 - r0, slices) for r0, r1 in units] == ranges
        empty = sum(r0 >= r1 for rr in ranges for r0, r1 in rr)
        assert empty == (1 if rows == 200 else 0)
        if rows:
            assert chunks >= 2 and all(sum(r0 < r1 for r0, r1 in rr) >= 2 for rr in ranges)
        # the carry: slices' low words that add up to 2^64 or more wrap at some add that meets a
        # non-zero old value, whatever the order; without the carry sq_hi would be the sum of the
        # slices' high words alone
        carried, top = 0, 0
        for p in range(P):
            whole = [sum(T.sq_of(x) for x in recs[c0 + r0:c0 + r1, p]) for (c0, _), rr in zip(units, ranges)
                     for r0, r1 in rr if r0 < r1]
            low = T.slice_low_words(recs, p, units, slices)
            assert low == [x & T.M64 for x in whole] and len(low) >= 3
            if sum(low) >= 2**64:
                carried += 1
                top = max(top, sum(low))
                assert sum(x >> 64 for x in whole) < sum(whole) >> 64 == int(T.aggregate(recs[:, p:p + 1])["sq_hi"][0])
        assert (carried, top >> 64) == MANY_ROWS_CARRY[name], (rows, carried, top)


def test_wide_grids_reach_the_wide_reduction_blocks(plan):
    """test_gpu_tradestats.test_wide_grids: 128 threads for P = 100, two blocks of 256 for P = 272,
    whose second block has threads past P; one slice, and three chunks at one row per chunk."""
    want = {"p100": (100, 128, 1), "p272": (272, 256, 2)}
    assert set(want) == set(T.WIDE_GRIDS)
    for name, (P, block, pblocks) in want.items():
        grid, series, recs = T.wide_grid_refs(name)
        assert grid.n_params == P == recs.shape[1] and [len(s[2]) for s in series] == [65, 130, 300]
        pl = plan(3, P)
        assert (pl["agg_block"], pl["agg_pblocks"], pl["agg_slices"], pl["chunks"]) == (block, pblocks, 1, 1)
        one = plan(3, P, 0, 256, T.rows_budget(P, 1))
        assert (one["per_chunk"], one["chunks"], one["agg_block"], one["agg_pblocks"]) == (1, 3, block, pblocks)
        # every parameter trades on some row, the parameters of the last block included, and the
        # columns differ (all but one pair): a thread that took another's parameter would show
        assert (recs["n_trades"].sum(axis=0) > 0).all() and int(recs["n_trades"].sum()) >= 10 * P
        assert len({recs[:, p].tobytes() for p in range(P)}) >= P - 1
        if pblocks == 2:
            assert recs[:, block - 1].tobytes() != recs[:, block].tobytes() != recs[:, 0].tobytes()
    assert 64 < 100 <= 128 and 272 >= 257 and 272 % 64 == 16 and 2 * 256 - 272 == 240


def test_plan_driver_under_asan_and_ubsan():
    exe = build_plan_driver("tstats_plan_driver", sanitize=True)
    for name in ("one_row_chunks", "list_small_budget"):
        units, P, lst, req = PLAN_SHAPES[name]
        assert run_driver(exe, units, P, lst, 256, req, sanitized=True) == \
            run_driver(build_plan_driver("tstats_plan_driver"), units, P, lst, 256, req)


# ---------------------------------------------------------------------- (e) under the sanitizers
RULES = ("no dataset loaded", "n = -1 outside [0, 1048576]", "n = 1048577 outside [0, 1048576]",
         "n = 3 with lanes == NULL (all-lanes mode takes n = 0)", "agg given in list mode (n = 3 lanes): it must be NULL",
         "out is required in list mode (n = 3 lanes)", "out and agg are both NULL", "", "", "",
         "P = 400 records of one row (51200 bytes) exceed the staging budget of 1000 bytes")
REFUSED = ("n_trades = -1 ", "n_bars = 0 ", "out is NULL", "equity is NULL", "trades is NULL", "outside the 2 bars",
           "side 0", "S = -1 ", "P = 0 ", "agg is NULL", "recs is NULL", "world = 0 ", "P = 0 ", "in and out")


def test_host_code_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ missing")
    exe = str(tmp_path / "tstats_asan")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", CSRC,
                        os.path.join(ROOT, "tests", "asan", "tstats_driver.cpp"),
                        os.path.join(CSRC, "tstats.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    # verify_asan_link_order=0: the environment may preload a library ahead of the ASan runtime
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0")
    traded = 0
    for strategy, seed in (("sma", 0), ("ema_ols", 1), ("boll", 2)):
        c, rf = RC.lane_case(strategy, seed), RC.lane_refs(strategy, seed)
        recs, agg = T.random_refs(strategy, seed)
        S, P = recs.shape
        fin, fout = str(tmp_path / f"in_{strategy}"), str(tmp_path / f"out_{strategy}")
        with open(fin, "wb") as f:
            f.write(np.array([S, P], np.int32).tobytes())
            for s in range(S):
                for p in range(P):
                    tr, eq = rf.lanes[s][p][1], rf.curves[s][p][1]
                    tr = np.zeros(0, D.TRADE_DTYPE) if tr is None else np.ascontiguousarray(tr, D.TRADE_DTYPE)
                    f.write(np.array([len(tr), len(eq)], np.int32).tobytes() + tr.tobytes()
                            + np.ascontiguousarray(eq, np.int64).tobytes())
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
        raw = open(fout, "rb").read()
        nr, na = S * P * 128, P * 136
        assert len(raw) == nr + 2 * na
        T.assert_same(np.frombuffer(raw[:nr], D.TSTATS_DTYPE).reshape(S, P), recs, f"{strategy}: records")
        T.assert_same(np.frombuffer(raw[nr:nr + na], D.TSTATS_AGG_DTYPE), agg, f"{strategy}: aggregate")
        T.assert_same(np.frombuffer(raw[nr + na:], D.TSTATS_AGG_DTYPE), agg, f"{strategy}: merged halves")
        traded += int(recs["n_trades"].sum())
        lines = r.stdout.splitlines()
        assert lines[-1] == f"ok {S} {P}"
        refused = [ln for ln in lines if ln.startswith("refused: ")]
        assert len(refused) == len(REFUSED)
        for ln, named in zip(refused, REFUSED):
            assert named in ln, ln
        assert [ln[len("rule: "):] for ln in lines if ln.startswith("rule: ")] == list(RULES)
    assert traded >= 500
