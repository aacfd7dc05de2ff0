"""Net of costs on the GPU (bt_costs, k_costs.hip; docs/costs_spec.md), every record and aggregate
field for field against the Python-int reference of costs_ref.py, which works from the C oracle's
complete trade lists and the curves rebuilt from them: the random cases of random_cases.py
(all-lanes and list mode, the aggregate alone, one row per chunk, the identities with the run's
summaries and with the trade statistics), ragged rows, the doubling cycles of limit_cases family A
at the limit level (sums of squares past 2^64; 205 rows in several slices and chunks), ladders of
1, 2 and 16 levels, crafted series of 130 bars that pin one rule each, the refusals and the derived
figures. There is no tolerance anywhere: every output is an integer.
tests/test_costs_cpu.py holds the host restatements to the same reference and proves that the cases
and levels reach the shapes the accounting can get wrong."""
import numpy as np
import pytest

import dbx_amd as D
import costs_ref as R
import random_cases as RC
import tradestats_ref as T

pytestmark = pytest.mark.gpu

LEVELS = R.LEVELS
assert LEVELS == ((0, 0), (1, 0), (0, 5), (7, 13), (2**20, 1000))


def _load(e, strategy, series, ids=None):
    """series: [(h, l, c)]."""
    closes = [s[2] for s in series]
    if strategy == "boll":
        e.load_ohlc(closes, [s[0] for s in series], [s[1] for s in series], sym_ids=ids)
    else:
        e.load_ohlc(closes, sym_ids=ids)


def _check_all_lanes(e, recs, levels, where):
    """All-lanes mode against the reference array: records, aggregate, the aggregate alone, and the
    same bytes with one row per chunk."""
    agg = R.aggregate(recs)
    _, P, C = recs.shape
    cs = e.costs(levels, params=True)
    R.assert_same(cs.lanes, recs, f"{where}: all-lanes records")
    R.assert_same(cs.params, agg, f"{where}: aggregate")
    assert cs.levels.tolist() == [list(lv) for lv in levels]
    only = e.costs(levels, per_lane=False, params=True)
    assert only.lanes is None and only.params.tobytes() == cs.params.tobytes(), f"{where}: agg alone"
    e.set_costs_budget(R.rows_budget(P, C, 1))
    try:
        one = e.costs(levels, params=True)
        one_only = e.costs(levels, per_lane=False, params=True)
    finally:
        e.set_costs_budget(0)
    assert one.lanes.tobytes() == cs.lanes.tobytes(), f"{where}: records, one row per chunk"
    assert one.params.tobytes() == cs.params.tobytes(), f"{where}: aggregate, one row per chunk"
    assert one_only.params.tobytes() == cs.params.tobytes(), f"{where}: aggregate alone, one row per chunk"
    return cs


# ------------------------------------------------------------------------ 1. the random cases
@pytest.mark.parametrize("strategy,seed", RC.CASES)
def test_random_cases(strategy, seed):
    c = RC.lane_case(strategy, seed)
    recs, _ = R.random_refs(strategy, seed)
    where = f"{strategy} seed {seed}"
    P = c.grid.n_params
    row = {i: s for s, i in enumerate(c.ids)}
    with D.Engine(c.grid, topk=c.topk) as e:
        _load(e, strategy, c.series, c.ids)
        e.run()
        before = (e.summaries().tobytes(), e.read_topk().tobytes())
        cs = _check_all_lanes(e, recs, LEVELS, where)
        # list mode: every lane shuffled, a tenth of them twice
        want = np.array([recs[row[sym], p] for sym, p in c.replay_lanes], D.COST_DTYPE)
        got = e.costs(LEVELS, c.replay_lanes)
        assert got.params is None
        R.assert_same(got.lanes, want, f"{where}: list mode")
        e.set_costs_budget(R.rows_budget(P, len(LEVELS), 1))
        try:
            small = e.costs(LEVELS, c.replay_lanes)
        finally:
            e.set_costs_budget(0)
        assert small.lanes.tobytes() == got.lanes.tobytes(), f"{where}: list mode under a small budget"
        # the identities with what the sweep kernels and the trade statistics produce
        summ, ts = e.summaries(), e.trade_stats().lanes
        free, one = cs.lanes[:, :, 0], cs.lanes[:, :, 1]
        for f in ("pnl", "mdd", "n_trades"):
            assert np.array_equal(free[f], summ[f]), f"{where}: {f} against summaries()"
        for mine, theirs in (("n_win", "n_win"), ("n_loss", "n_loss"), ("win_sum", "gross_win"),
                             ("loss_sum", "gross_loss"), ("mdd_bar", "mdd_bar"), ("underwater_bars", "underwater_bars")):
            assert np.array_equal(free[mine], ts[theirs]), f"{where}: {mine} against trade_stats()"
        assert np.array_equal(one["fees"], 2 * summ["n_trades"].astype(np.int64)), f"{where}: fees at (1, 0)"
        assert np.array_equal(cs.lanes["win_sum"] - cs.lanes["loss_sum"], cs.lanes["pnl"]), where
        for j in range(len(LEVELS)):
            assert np.array_equal(cs.lanes[:, :, j]["pnl"] + cs.lanes[:, :, j]["fees"], summ["pnl"]), f"{where}: level {j}"
            assert np.array_equal(cs.lanes[:, :, j]["turnover"], free["turnover"]), f"{where}: level {j}"
        # s2 at the free level is the one-lane portfolio's, on a handful of lanes
        for sym, p in c.replay_lanes[:5]:
            pf = e.portfolio([(sym, p)]).summary
            r = free[row[sym], p]
            assert (int(r["s2_lo"]), int(r["s2_hi"])) == (int(pf["s2_lo"]), int(pf["s2_hi"])), f"{where}: s2 of {sym, p}"
        assert (e.summaries().tobytes(), e.read_topk().tobytes()) == before, f"{where}: the run's results changed"


# ------------------------------------------------------------------------------ 2. ragged rows
@pytest.mark.parametrize("strategy", RC.STRATEGIES)
def test_ragged_rows(strategy):
    series = T.ragged_series(strategy)
    grid = T.RAGGED_GRIDS[strategy]()
    recs = R.case_series(strategy, grid, series, LEVELS)
    assert recs["n_bars"][:, 0, 0].tolist() == list(T.RAGGED) and int(recs["n_trades"][:, :, 0].sum()) >= 50
    zero = np.zeros((), D.COST_DTYPE)     # the 1-bar row: all zeros but n_bars and mdd_bar
    zero["n_bars"], zero["mdd_bar"] = 1, -1
    with D.Engine(grid) as e:
        _load(e, strategy, series)
        cs = _check_all_lanes(e, recs, LEVELS, f"{strategy} ragged rows")
        assert all(x.tobytes() == zero.tobytes() for x in cs.lanes[0].reshape(-1))


# --------------------------------------------------------------------------------- 3. family A
@pytest.mark.parametrize("name", ("sma", "ema_ols", "boll"))
def test_family_a_at_the_limit_level(name):
    """Prices near 2^31 under (2^20, 1000): fees near 2^29 a fill, increments near 2^32, sums of
    their squares past 2^64 (tests/test_costs_cpu.py counts the lanes)."""
    grid, series, recs = R.family_a_refs(name)
    if name != "ema_ols":
        assert sum(R.s2_of(x) >= 2**64 for x in recs.reshape(-1)) >= 10
    with D.Engine(grid) as e:
        _load(e, name, [(h, lo, c) for c, h, lo in series])
        cs = e.costs(R.LIMIT, params=True)
    R.assert_same(cs.lanes, recs, f"family A {name}: records")
    R.assert_same(cs.params, R.aggregate(recs), f"family A {name}: aggregate")
    assert cs.s2.tolist() == [[[R.s2_of(x) for x in lane] for lane in row] for row in recs]


@pytest.mark.parametrize("name", ("sma", "boll"))
def test_family_a_many_rows_in_slices_and_chunks(name):
    """Family A repeated to 205 rows: cost_agg_kernel with grid y = 4 at the default budget, as
    chunks of 100, 100 and 5 rows of two slices each, and as chunks of 200 and 5 rows of four slices
    whose last is empty in the short chunk (tests/test_costs_cpu.py holds the plan to these)."""
    grid, series, recs = R.family_a_many_rows(name)
    agg = R.aggregate(recs)
    P = grid.n_params
    with D.Engine(grid) as e:
        _load(e, name, [(h, lo, c) for c, h, lo in series])
        for rows in (0,) + T.A_CHUNK_ROWS:
            where = f"family A {name} x {T.A_ROWS} rows, {rows or 'all'} rows per chunk"
            e.set_costs_budget(R.rows_budget(P, 1, rows) if rows else 0)
            try:
                cs = e.costs(R.LIMIT, params=True)
                only = e.costs(R.LIMIT, per_lane=False, params=True)
            finally:
                e.set_costs_budget(0)
            R.assert_same(cs.lanes, recs, f"{where}: records")
            R.assert_same(cs.params, agg, f"{where}: aggregate")
            assert only.lanes is None
            R.assert_same(only.params, agg, f"{where}: aggregate alone")


# ------------------------------------------------------------------- 4. ladders of 1, 2, 16 levels
SIXTEEN = tuple((3 * j * j + (j % 3), (61 * j) % 1001) for j in range(15)) + ((2**20, 1000),)
assert len(set(SIXTEEN)) == 16 and SIXTEEN[0] == (0, 0)


@pytest.mark.parametrize("strategy", RC.STRATEGIES)
def test_ladders_of_one_two_and_sixteen_levels(strategy):
    """Level j's record depends on level j alone: 16 distinct levels against the reference, the same
    16 in reverse order giving the reversed records, one level alone, and a level repeated."""
    seed = 3
    c = RC.lane_case(strategy, seed)
    recs, _ = R.random_refs(strategy, seed, SIXTEEN)
    assert len({recs[:, :, j].tobytes() for j in range(16)}) == 16, "the 16 levels give 16 different answers"
    with D.Engine(c.grid) as e:
        _load(e, strategy, c.series, c.ids)
        cs = _check_all_lanes(e, recs, SIXTEEN, f"{strategy}: 16 levels")
        rev = e.costs(SIXTEEN[::-1], params=True)
        assert rev.lanes.tobytes() == np.ascontiguousarray(cs.lanes[:, :, ::-1]).tobytes(), "reversed levels"
        assert rev.params.tobytes() == np.ascontiguousarray(cs.params[:, ::-1]).tobytes(), "reversed levels, aggregate"
        for j in (0, 7, 15):
            one = e.costs([SIXTEEN[j]], params=True)
            assert one.lanes.shape[2] == 1 and one.lanes[:, :, 0].tobytes() == np.ascontiguousarray(cs.lanes[:, :, j]).tobytes()
            assert one.params[:, 0].tobytes() == np.ascontiguousarray(cs.params[:, j]).tobytes()
        two = e.costs([SIXTEEN[5], SIXTEEN[5]], params=True)
        assert two.lanes[:, :, 0].tobytes() == two.lanes[:, :, 1].tobytes() == np.ascontiguousarray(cs.lanes[:, :, 5]).tobytes()
        assert two.params[:, 0].tobytes() == two.params[:, 1].tobytes()
        lst = e.costs(SIXTEEN, c.replay_lanes[:7])
        row = {i: s for s, i in enumerate(c.ids)}
        R.assert_same(lst.lanes, np.array([recs[row[sym], p] for sym, p in c.replay_lanes[:7]], D.COST_DTYPE), "list, 16 levels")


# ---------------------------------------------------------------------------- 5. crafted series
MOMENTUM = 0   # param 0 of the crafted grid: SMA(1, 2), long after an up bar, short after a down bar


def _craft_grid():
    return D.Grid.sma([1, 2], [2, 5])


def _plain(c):
    c = np.asarray(c, np.int32)
    return (c, c, c)


def _steps(start, moves):
    """Closes from a start and one move per bar after it."""
    return np.concatenate([[start], start + np.cumsum(moves)]).astype(np.int32)


def test_crafted_fills_at_the_tile_edge():
    """130 bars of SMA(1, 2): rising, one down bar at 63 (a flip at lane 63), an up bar at 64 (a flip
    at lane 0 of the next tile: the short entered at 63 exits at 64), rising to the forced exit at
    129; and 65 rising bars whose only exit is the forced one at B - 1 = 64."""
    moves = np.full(129, 10)
    moves[62] = -25                 # c_63 < c_62
    a = _steps(50_000, moves)
    b = _steps(70_000, np.full(64, 7))
    assert len(a) == 130 and len(b) == 65 and a[63] < a[62] and a[64] > a[63]
    series = [_plain(a), _plain(b)]
    grid = _craft_grid()
    lanes = R.case_lanes("sma", grid, series)
    tr = lanes[0][MOMENTUM][0]
    assert [(e, x) for e, x, _, _, _ in tr] == [(1, 63), (63, 64), (64, 129)], tr
    assert [(e, x) for e, x, _, _, _ in lanes[1][MOMENTUM][0]] == [(1, 64)]
    recs = R.case_series("sma", grid, series, LEVELS, lanes)
    # one fee per fill: six fills and two; the flip bars carry two of them
    assert recs[0, MOMENTUM, 1]["fees"] == 6 and recs[1, MOMENTUM, 1]["fees"] == 2
    assert R.bar_fees(tr, (1, 0)) == {1: 1, 63: 2, 64: 2, 129: 1}
    with D.Engine(grid) as e:
        _load(e, "sma", series)
        _check_all_lanes(e, recs, LEVELS, "crafted tile edge")


def test_crafted_entry_fee_and_equal_net_drawdowns():
    """SMA(1, 2) on plateaus (no signal on a flat bar: the position is held). At (1, 0): the entry
    at bar 2 pays 1 while the gross equity has not moved, so bar 2 is the first bar under water; a
    3-tick move against the position with the 2 ticks of the flip makes a net drawdown of 5 at bar 4
    and again at bar 70, one tile later: the first is mdd_bar."""
    c = [1000, 1000, 1001, 1004, 1001, 998, 990] + [990] * 63 + [993, 1010] + [1010] * 58
    assert len(c) == 130
    series = [_plain(c)]
    grid = _craft_grid()
    lanes = R.case_lanes("sma", grid, series)
    tr, eq = lanes[0][MOMENTUM]
    assert [(e, x, s) for e, x, s, _, _ in tr] == [(2, 4, 1), (4, 70, -1), (70, 129, 1)], tr
    N = R.net_curve(tr, eq, (1, 0))
    peak = np.maximum.accumulate(np.maximum(N, 0))
    dd = (peak - np.array(N)).tolist()
    assert eq[:3] == [0, 0, 0] and N[:3] == [0, 0, -1] and max(dd) == 5 and [t for t, x in enumerate(dd) if x == 5] == [4, 70]
    recs = R.case_series("sma", grid, series, LEVELS, lanes)
    r = recs[0, MOMENTUM, 1]
    assert (int(r["mdd"]), int(r["mdd_bar"])) == (5, 4) and 4 // 64 != 70 // 64
    g = recs[0, MOMENTUM, 0]
    assert int(g["underwater_bars"]) < int(r["underwater_bars"]) and int(g["mdd"]) == 3
    with D.Engine(grid) as e:
        _load(e, "sma", series)
        _check_all_lanes(e, recs, LEVELS, "crafted drawdowns")


def test_crafted_bollinger_stop_and_target_fill_prices():
    """h = l = c: a long entered on a drop is stopped out when the drop goes on, at the stop level
    and not at the close; one entered before a bounce leaves at the target level. The fee of the
    exit is taken on the level price."""
    cyc = [100_000] * 8 + [90_000, 80_000] + [80_000] * 7 + [70_000, 77_000] + [77_000] * 7
    c = np.array((cyc * 6)[:130], np.int32)
    series = [_plain(c)]
    grid = D.Grid.boll([5], [2], [50], [50, 9000], k_den=2)
    lanes = R.case_lanes("boll", grid, series)
    tr = lanes[0][0][0]
    stops = [(x, xpx) for e, x, s, epx, xpx in tr if s * (xpx - epx) < 0 and xpx != int(c[x])]
    targets = [(x, xpx) for e, x, s, epx, xpx in tr if s * (xpx - epx) > 0 and xpx != int(c[x])]
    assert len(stops) >= 3 and len(targets) >= 3, (stops, targets)
    lv = (0, 1000)                  # 10 %: the fee differs between level price and close
    assert all(R.fee(xpx, lv) != R.fee(int(c[x]), lv) for x, xpx in stops + targets)
    levels = LEVELS + (lv,)
    recs = R.case_series("boll", grid, series, levels, lanes)
    with D.Engine(grid) as e:
        _load(e, "boll", series)
        _check_all_lanes(e, recs, levels, "crafted Bollinger fills")


# ------------------------------------------------------------------------------- 6. refusals
def test_refusals_name_the_value_and_leave_the_engine_usable():
    grid = D.Grid.sma([2, 4], [8, 16, 30])
    P = grid.n_params
    f = D.engine.sym("bt_costs")
    out = np.zeros(4 * P * 16, D.COST_DTYPE)
    agg = np.zeros(P * 16, D.COST_AGG_DTYPE)
    lanes = np.zeros(3, D.LANE_DTYPE)
    lv = np.array(LEVELS, np.int32)
    keep = []

    def levels(*pairs):
        a = np.array(pairs, np.int32)
        keep.append(a)
        return a.ctypes.data

    def last():
        return D.lib().bt_last_error().decode()

    with D.Engine(grid) as e:
        h = e._h
        o, a, l5, ln = out.ctypes.data, agg.ctypes.data, lv.ctypes.data, lanes.ctypes.data
        assert f(h, 5, l5, 0, None, o, None) == -1 and "bt_costs: no dataset loaded" in last()
        e.load_synthetic(0x5EED, 40, 4, 300, D.BT_DAILY)
        want = e.costs(LEVELS, params=True)
        assert int(want.lanes["n_trades"].sum()) > 0
        lanes["sym"], lanes["param"] = (40, 43, 41), (0, P - 1, 2)
        for args, named in (
            ((0, l5, 0, None, o, None), "C = 0 outside [1, 16]"),
            ((17, l5, 0, None, o, None), "C = 17 outside [1, 16]"),
            ((5, None, 0, None, o, None), "levels is NULL"),
            ((2, levels((0, 0), ((1 << 20) + 1, 0)), 0, None, o, None), "level 1: fixed = 1048577 outside [0, 1048576]"),
            ((2, levels((0, 1001), (0, 0)), 0, None, o, None), "level 0: bps = 1001 outside [0, 1000]"),
            ((2, levels((-1, 0), (0, 0)), 0, None, o, None), "level 0: fixed = -1 outside"),
            ((2, levels((0, 0), (0, -1)), 0, None, o, None), "level 1: bps = -1 outside"),
            ((5, l5, -1, ln, o, None), "n = -1 outside [0, 1048576]"),
            ((5, l5, (1 << 20) + 1, ln, o, None), "n = 1048577 outside [0, 1048576]"),
            ((5, l5, 3, None, o, None), "n = 3 with lanes == NULL"),
            ((5, l5, 3, ln, o, a), "agg given in list mode (n = 3 lanes)"),
            ((5, l5, 3, ln, None, None), "out is required in list mode (n = 3 lanes)"),
            ((5, l5, 0, None, None, None), "out and agg are both NULL"),
        ):
            assert f(h, *args) == -1
            assert last().startswith("bt_costs: ") and named in last(), last()
        with pytest.raises(D.BtError, match=r"unknown symbol id 44 \(lane 1\)"):
            e.costs(LEVELS, [(40, 0), (44, 0)])
        with pytest.raises(D.BtError, match=rf"param {P} outside \[0, {P}\) \(lane 2\)"):
            e.costs(LEVELS, [(40, 0), (41, 1), (42, P)])
        with pytest.raises(ValueError, match="leave lanes out"):
            e.costs(LEVELS, [(40, 0)], params=True)
        with pytest.raises(D.BtError, match=r"C = 0 outside \[1, 16\]"):
            e.costs([])
        e.set_costs_budget(P * 5 * 88)
        with pytest.raises(D.BtError, match=rf"P \* C = {P} \* 5 records of one row \({P * 5 * 88} bytes\) exceed the "
                                            rf"staging budget of {P * 5 * 88} bytes"):
            e.costs(LEVELS)
        with pytest.raises(D.BtError, match="bytes = -5 is negative"):
            e.set_costs_budget(-5)
        e.set_costs_budget(0)
        assert f(None, 5, l5, 0, None, o, None) == -1 and "bt_costs: null engine" in last()
        # list mode with no lane is legal and touches nothing
        assert f(h, 5, l5, 0, ln, None, None) == 0 and e.costs(LEVELS, []).lanes.shape == (0, 5)
        # the engine is usable afterwards, and says what it said before
        again = e.costs(LEVELS, params=True)
        assert again.lanes.tobytes() == want.lanes.tobytes() and again.params.tobytes() == want.params.tobytes()
        got = e.costs(LEVELS, [(40, 0), (43, P - 1), (41, 2), (40, 0)]).lanes
        assert got.tobytes() == want.lanes[[0, 3, 1, 0], [0, P - 1, 2, 0]].tobytes()


# ----------------------------------------------------------------------- 7. the derived figures
def test_derived_figures():
    strategy, seed = "sma", 1
    c = RC.lane_case(strategy, seed)
    recs, agg = R.random_refs(strategy, seed)
    with D.Engine(c.grid) as e:
        _load(e, strategy, c.series, c.ids)
        cs = e.costs(LEVELS, params=True)
    R.assert_same(cs.lanes, recs, "records")
    f8 = np.float64

    def ratio(a, b):
        return np.array([float(x) / float(y) if y else 0.0 for x, y in zip(a.reshape(-1).tolist(), b.reshape(-1).tolist())],
                        f8).reshape(a.shape)

    assert np.array_equal(cs.win_rate(), ratio(recs["n_win"], recs["n_trades"]))
    assert np.array_equal(cs.profit_factor(), ratio(recs["win_sum"], recs["loss_sum"]))
    gross = recs["pnl"] + recs["fees"]
    assert np.array_equal(cs.breakeven_fixed(), ratio(gross, 2 * recs["n_trades"].astype(np.int64)))
    assert np.array_equal(cs.breakeven_bps(), ratio(gross.astype(f8) * 10000.0, recs["turnover"]))
    assert np.array_equal(cs.survivors(), ratio(agg["n_profit"], agg["n_sym"]))
    for j in range(len(LEVELS)):
        order = sorted(range(agg.shape[0]), key=lambda p: (-int(agg["pnl"][p, j]), p))
        assert cs.rank(j).tolist() == order and cs.rank(j, 3).tolist() == order[:3]
    # net_sharpe: the formula of docs/portfolio_spec.md in Python floats, one operation at a time
    sh = cs.net_sharpe(c.grid.annualization)
    for idx in np.ndindex(recs.shape):
        r = recs[idx]
        n = float(r["n_bars"])
        m = float(int(r["pnl"])) / n
        v = float(R.s2_of(r)) / n - m * m
        want = (m / np.sqrt(v)) * np.sqrt(float(c.grid.annualization)) if v > 0 else 0.0
        assert sh[idx] == want, idx
