"""Per-lane trade statistics on the GPU (bt_trade_stats, k_tstats.hip; docs/tradestats_spec.md),
every record and aggregate field for field against the Python-int reference of tradestats_ref.py,
which works from the C oracle's complete trade lists and the curves rebuilt from them: the random
cases of random_cases.py (all-lanes and list mode, one row per chunk, the identities with the run's
summaries), ragged rows, the doubling cycles of limit_cases family A (sums of squares past 2^64),
the reduction's geometry (family A repeated to 205 rows: several slices, several chunks, an empty
trailing slice, sums of squares whose low words wrap between the slices' atomic adds; grids of 100
and 272 parameters: reduction blocks of 128 and 256 threads, two blocks along p), crafted series
that pin the drawdown and streak rules, and the refusals.
tests/test_tradestats_cpu.py holds the host restatements to the same reference and proves that the
cases reach the shapes the accounting and the reduction can get wrong.
tests/test_gpu_tstats_boot_limits.py runs the limit families B, C and D; tests/test_gpu_random_lanes.py
runs the call among the other analysis calls on one engine."""
import numpy as np
import pytest

import dbx_amd as D
import random_cases as RC
import tradestats_ref as T

pytestmark = pytest.mark.gpu


def _load(e, strategy, series, ids=None):
    """series: [(h, l, c)]."""
    closes = [s[2] for s in series]
    if strategy == "boll":
        e.load_ohlc(closes, [s[0] for s in series], [s[1] for s in series], sym_ids=ids)
    else:
        e.load_ohlc(closes, sym_ids=ids)


def _one_row_budget(P):
    """plan_tstats: agg[P] rounded up to 256 bytes, one rounding of the records, one row of P."""
    return (P * D.TSTATS_AGG_DTYPE.itemsize + 255) // 256 * 256 + 256 + P * D.TSTATS_DTYPE.itemsize


def _check_all_lanes(e, recs, where):
    """All-lanes mode against the reference matrix: records, aggregate, each output alone, and the
    same bytes with one row per chunk."""
    agg = T.aggregate(recs)
    ts = e.trade_stats(params=True)
    T.assert_same(ts.lanes, recs, f"{where}: all-lanes records")
    T.assert_same(ts.params, agg, f"{where}: aggregate")
    only = e.trade_stats(per_lane=False, params=True)
    assert only.lanes is None and only.params.tobytes() == ts.params.tobytes(), f"{where}: agg alone"
    e.set_tstats_budget(_one_row_budget(recs.shape[1]))
    try:
        one = e.trade_stats(params=True)
    finally:
        e.set_tstats_budget(0)
    assert one.lanes.tobytes() == ts.lanes.tobytes(), f"{where}: records, one row per chunk"
    assert one.params.tobytes() == ts.params.tobytes(), f"{where}: aggregate, one row per chunk"
    return ts


# ------------------------------------------------------------------------ 1. the random cases
@pytest.mark.parametrize("strategy,seed", RC.CASES)
def test_random_cases(strategy, seed):
    c = RC.lane_case(strategy, seed)
    recs, _ = T.random_refs(strategy, seed)
    where = f"{strategy} seed {seed}"
    P = c.grid.n_params
    row = {i: s for s, i in enumerate(c.ids)}
    with D.Engine(c.grid, topk=c.topk) as e:
        _load(e, strategy, c.series, c.ids)
        e.run()
        before = (e.summaries().tobytes(), e.read_topk().tobytes())
        ts = _check_all_lanes(e, recs, where)
        # list mode: every lane shuffled, a tenth of them twice
        want = np.array([recs[row[sym], p] for sym, p in c.replay_lanes], D.TSTATS_DTYPE)
        got = e.trade_stats(c.replay_lanes)
        assert got.params is None
        T.assert_same(got.lanes, want, f"{where}: list mode")
        e.set_tstats_budget(_one_row_budget(P))
        try:
            small = e.trade_stats(c.replay_lanes)
        finally:
            e.set_tstats_budget(0)
        assert small.lanes.tobytes() == got.lanes.tobytes(), f"{where}: list mode under a small budget"
        # the identities with what the sweep kernels produce
        summ = e.summaries()
        for f in ("n_trades", "mdd", "hash"):
            assert np.array_equal(ts.lanes[f], summ[f]), f"{where}: {f} against summaries()"
        assert np.array_equal(ts.lanes["gross_win"] - ts.lanes["gross_loss"], summ["pnl"]), f"{where}: pnl"
        assert np.array_equal(ts.lanes["hold_sum"], summ["exposure"]), f"{where}: exposure"
        assert (e.summaries().tobytes(), e.read_topk().tobytes()) == before, f"{where}: the run's results changed"


# ------------------------------------------------------------------------------ 2. ragged rows
RAGGED, RAGGED_GRIDS = T.RAGGED, T.RAGGED_GRIDS   # shared with the window edges of test_gpu_bootstrap.py


@pytest.mark.parametrize("strategy", RC.STRATEGIES)
def test_ragged_rows(strategy):
    series = T.ragged_series(strategy)
    grid = RAGGED_GRIDS[strategy]()
    recs = T.case_series(strategy, grid, series)
    assert recs["n_bars"][:, 0].tolist() == list(RAGGED) and int(recs["n_trades"].sum()) >= 50
    # the 1-bar row: all zeros but n_bars, and no drawdown bars
    zero = np.zeros((), D.TSTATS_DTYPE)
    zero["n_bars"], zero["mdd_bar"], zero["peak_bar"] = 1, -1, -1
    assert all(x.tobytes() == zero.tobytes() for x in recs[0])
    with D.Engine(grid) as e:
        _load(e, strategy, series)
        ts = _check_all_lanes(e, recs, f"{strategy} ragged rows")
        assert all(x.tobytes() == zero.tobytes() for x in ts.lanes[0])


# --------------------------------------------------------------------------------- 3. family A
@pytest.mark.parametrize("name", ("sma", "ema_ols", "boll"))
def test_family_a_doubling_cycles(name):
    grid, series, recs = T.family_a_refs(name)
    if name == "boll":   # sums of squares that leave int64
        assert sum(T.sq_of(x) >= 2**64 for x in recs.reshape(-1)) >= 100
    with D.Engine(grid) as e:
        _load(e, name, [(h, lo, c) for c, h, lo in series])
        ts = e.trade_stats(params=True)
    T.assert_same(ts.lanes, recs, f"family A {name}: records")
    T.assert_same(ts.params, T.aggregate(recs), f"family A {name}: aggregate")
    assert ts.sq.tolist() == [[T.sq_of(x) for x in r] for r in recs]


# --------------------------------------------------------------- 3b. the reduction's geometry
@pytest.mark.parametrize("name", ("sma", "boll"))
def test_family_a_many_rows_in_slices_and_chunks(name):
    """Family A repeated to 205 rows: tstats_agg_kernel with grid y = 4 at the default budget, as
    chunks of 100, 100 and 5 rows of two slices each, and as chunks of 200 and 5 rows of four slices
    whose last is empty in the short chunk. The sums of squares wrap 2^64 between the slices' atomic
    adds (tests/test_tradestats_cpu.py proves it from the reference), so the carry decides sq_hi.
    Measured on an MI355X, as pytest reports the case with its Python-int aggregates: below 0.07 s."""
    grid, series, recs = T.family_a_many_rows(name)
    agg = T.aggregate(recs)
    with D.Engine(grid) as e:
        _load(e, name, [(h, lo, c) for c, h, lo in series])
        for rows in (0,) + T.A_CHUNK_ROWS:
            where = f"family A {name} x {T.A_ROWS} rows, {rows or 'all'} rows per chunk"
            e.set_tstats_budget(T.rows_budget(grid.n_params, rows) if rows else 0)
            try:
                ts = e.trade_stats(params=True)
                only = e.trade_stats(per_lane=False, params=True)
            finally:
                e.set_tstats_budget(0)
            T.assert_same(ts.lanes, recs, f"{where}: records")
            T.assert_same(ts.params, agg, f"{where}: aggregate")
            assert only.lanes is None
            T.assert_same(only.params, agg, f"{where}: aggregate alone")


@pytest.mark.parametrize("name", list(T.WIDE_GRIDS))
def test_wide_grids(name):
    """P = 100 (one reduction block of 128 threads) and P = 272 (two blocks of 256, the second
    with threads past P) on rows of 65, 130 and 300 bars: both output modes and one row per chunk.
    Measured on an MI355X: below 0.07 s a case."""
    grid, series, recs = T.wide_grid_refs(name)
    with D.Engine(grid) as e:
        _load(e, "sma", series)
        _check_all_lanes(e, recs, f"wide grid {name}")


# ---------------------------------------------------------------------------- 4. crafted series
MOMENTUM = 0   # param 0 of CRAFT_GRID: SMA(1, 2), long after an up bar, short after a down bar


def _craft_grid():
    return D.Grid.sma([1, 2], [2, 5])


def _closes_for_equity(equity):
    """Closes on which SMA(1, 2) has the equity curve `equity` (E_0 = E_1 = 0, no two consecutive
    values equal after that): the lane holds the sign of the last move, so the next move is the
    wanted increment times that sign."""
    assert equity[0] == equity[1] == 0
    c = [1_000_000, 1_000_001]
    sign = 1
    for a, b in zip(equity[1:-1], equity[2:]):
        assert a != b
        move = (b - a) * sign
        c.append(c[-1] + move)
        sign = 1 if move > 0 else -1
    return np.array(c, np.int32)


def _path(*legs):
    """An equity curve from (target, bars) legs of equal steps, after E_0 = E_1 = 0."""
    e = [0, 0]
    for target, bars in legs:
        step, rem = divmod(target - e[-1], bars)
        assert rem == 0 and step != 0
        e += [e[-1] + step * (k + 1) for k in range(bars)]
    return e


def _plain(c):
    return (c, c, c)


def test_crafted_drawdown_rules():
    rising = np.arange(10_000, 10_000 + 10 * 200, 10, dtype=np.int32)                  # strictly rising closes
    flat = np.full(150, 77_777, np.int32)
    # up to 50 at bar 11, under water for 59 bars, back to exactly 50 at bar 71 (the next tile),
    # then down to -40 at bar 161
    tie = _path((50, 10), (-9, 59), (50, 1), (-40, 90))
    # 100 at bar 6, 60 at bar 26 (a drawdown of 40), 200 at bar 96, 160 at bar 116 (40 again, two
    # tiles later), 230 at the end
    twice = _path((100, 5), (60, 20), (200, 70), (160, 20), (230, 35))
    series = [_plain(rising), _plain(flat), _plain(_closes_for_equity(tie)), _plain(_closes_for_equity(twice))]
    grid = _craft_grid()
    recs = T.case_series("sma", grid, series)
    m = MOMENTUM
    # what each series is there for, from the reference alone
    assert not recs[0]["mdd"].any() and (recs[0]["mdd_bar"] == -1).all() and (recs[0]["peak_bar"] == -1).all()
    assert not recs[0]["underwater_bars"].any() and recs[0]["n_trades"].sum() >= 3 and (recs[0]["gross_win"] > 0).any()
    assert not recs[1]["n_trades"].any() and not recs[1]["mdd"].any() and (recs[1]["n_bars"] == 150).all()
    r = recs[2, m]
    assert (int(r["mdd"]), int(r["mdd_bar"]), int(r["peak_bar"])) == (90, 161, 11)     # not the tie's bar 71
    assert (int(r["underwater_bars"]), int(r["max_underwater"])) == (149, 90)           # 59 + 90: the tie ends the run
    r = recs[3, m]
    assert (int(r["mdd"]), int(r["mdd_bar"]), int(r["peak_bar"])) == (40, 26, 6)        # the first of the two
    assert 26 // 64 != 116 // 64
    with D.Engine(grid) as e:
        _load(e, "sma", series)
        _check_all_lanes(e, recs, "crafted drawdowns")


def test_crafted_bollinger_flat_trades_between_losses():
    """h = l = c plateaus: a long entered on a drop is stopped out when the drop goes on (a loss),
    and one entered on the last drop leaves at its entry price when the window has filled with the
    plateau (D = 0: a flat trade). Cycles of drop, plateau, drop give loss, flat, loss."""
    cyc = [100_000] * 8 + [90_000] + [80_000] * 7 + [70_000, 60_000] + [60_000] * 7
    c = np.array(cyc * 9, np.int32)
    series = [_plain(c)]
    grid = D.Grid.boll([5], [2], [50], [50, 9000], k_den=2)
    recs = T.case_series("boll", grid, series)
    from replay_ref import oracle_lane
    _, tr = oracle_lane("boll", grid, 0, series[0], cap=len(c))
    pnl = [side * (xpx - epx) for _, _, side, epx, xpx in T.trade_tuples(tr)]
    kinds = "".join("W" if x > 0 else "L" if x < 0 else "F" for x in pnl)
    assert "LFL" in kinds and kinds.count("F") >= 9, kinds
    r = recs[0, 0]
    assert int(r["n_trades"]) - int(r["n_win"]) - int(r["n_loss"]) == kinds.count("F")
    assert int(r["max_loss_streak"]) == max(len(x) for x in kinds.replace("W", "F").split("F")) < int(r["n_loss"])
    with D.Engine(grid) as e:
        _load(e, "boll", series)
        _check_all_lanes(e, recs, "crafted Bollinger plateaus")


# ------------------------------------------------------------------------------- 5. refusals
def test_refusals_name_the_value_and_leave_the_engine_usable():
    grid = D.Grid.sma([2, 4], [8, 16, 30])
    P = grid.n_params
    f = D.engine.sym("bt_trade_stats")
    out = np.zeros(4 * P, D.TSTATS_DTYPE)
    agg = np.zeros(P, D.TSTATS_AGG_DTYPE)
    lanes = np.zeros(3, D.LANE_DTYPE)

    def last():
        return D.lib().bt_last_error().decode()

    with D.Engine(grid) as e:
        h = e._h
        assert f(h, 0, None, out.ctypes.data, None) == -1 and "bt_trade_stats: no dataset loaded" in last()
        e.load_synthetic(0x5EED, 40, 4, 300, D.BT_DAILY)
        want = e.trade_stats(params=True)
        assert int(want.lanes["n_trades"].sum()) > 0
        lanes["sym"], lanes["param"] = (40, 43, 41), (0, P - 1, 2)
        for args, named in (
            ((-1, lanes.ctypes.data, out.ctypes.data, None), "n = -1 outside [0, 1048576]"),
            (((1 << 20) + 1, lanes.ctypes.data, out.ctypes.data, None), "n = 1048577 outside [0, 1048576]"),
            ((3, None, out.ctypes.data, None), "n = 3 with lanes == NULL"),
            ((3, lanes.ctypes.data, out.ctypes.data, agg.ctypes.data), "agg given in list mode (n = 3 lanes)"),
            ((3, lanes.ctypes.data, None, None), "out is required in list mode (n = 3 lanes)"),
            ((0, None, None, None), "out and agg are both NULL"),
        ):
            assert f(h, *args) == -1
            assert last().startswith("bt_trade_stats: ") and named in last(), last()
        with pytest.raises(D.BtError, match=r"unknown symbol id 44 \(lane 1\)"):
            e.trade_stats([(40, 0), (44, 0)])
        with pytest.raises(D.BtError, match=rf"param {P} outside \[0, {P}\) \(lane 2\)"):
            e.trade_stats([(40, 0), (41, 1), (42, P)])
        with pytest.raises(D.BtError, match="param -1 outside"):
            e.trade_stats([(40, -1)])
        with pytest.raises(ValueError, match="leave lanes out"):
            e.trade_stats([(40, 0)], params=True)
        e.set_tstats_budget(P * 128)
        with pytest.raises(D.BtError, match=rf"P = {P} records of one row \({P * 128} bytes\) exceed the staging "
                                            rf"budget of {P * 128} bytes"):
            e.trade_stats()
        with pytest.raises(D.BtError, match="bytes = -5 is negative"):
            e.set_tstats_budget(-5)
        e.set_tstats_budget(0)
        assert f(None, 0, None, out.ctypes.data, None) == -1 and "bt_trade_stats: null engine" in last()
        # list mode with no lane is legal and touches nothing
        assert f(h, 0, lanes.ctypes.data, None, None) == 0 and len(e.trade_stats([]).lanes) == 0
        # the engine is usable afterwards, and says what it said before
        again = e.trade_stats(params=True)
        assert again.lanes.tobytes() == want.lanes.tobytes() and again.params.tobytes() == want.params.tobytes()
        got = e.trade_stats([(40, 0), (43, P - 1), (41, 2), (40, 0)]).lanes
        assert got.tobytes() == want.lanes[[0, 3, 1, 0], [0, P - 1, 2, 0]].tobytes()
