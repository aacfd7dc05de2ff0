"""Lane replay on the GPU (bt_replay, k_replay.hip; Engine.replay): chosen (symbol, parameter)
lanes with their trades, position and equity curve, bit for bit against the C oracle and the
numpy curve reconstruction of replay_ref.py (pinned to the oracle in test_replay_cpu.py), and equal
to what the sweep kernels produce for the same lanes."""
import functools
import re

import numpy as np
import pytest

import dbx_amd as D
from dbx_amd import engine as E
from helpers import compare_summary, compare_summaries, compare_trades
from replay_ref import curves_from_trades, gen_hlc, oracle_lane

pytestmark = pytest.mark.gpu

CAP = 4096          # trades kept per replayed lane
ORC_CAP = 1 << 15   # the oracle's lists are complete (the curves are rebuilt from them)
STRATEGIES = ("sma", "ema_ols", "boll")


def _load(e, strategy, series, ids=None):
    """series: [(h, l, c)]"""
    if strategy == "boll":
        e.load_ohlc([s[2] for s in series], [s[0] for s in series], [s[1] for s in series], sym_ids=ids)
    else:
        e.load_ohlc([s[2] for s in series], sym_ids=ids)


def _check_lane(rp, i, strategy, grid, p, ohlc, where, cap=CAP):
    """Row i of a replay against the oracle: summary, n_bars, whole trade list, and the curves
    when the replay has them (zero past the symbol's bars)."""
    s, tr = oracle_lane(strategy, grid, p, ohlc, cap=ORC_CAP)
    n = int(s["n_trades"])
    assert n <= ORC_CAP, where
    compare_summary(rp.summaries[i], s, where)
    bars = len(ohlc[2])
    assert int(rp.n_bars[i]) == bars, where
    if rp.trades is not None:
        compare_trades(rp.trades[i], tr, min(n, cap), where)
        assert not rp.trades[i, min(n, cap):].view(np.uint8).any(), f"{where}: trade row not zero past the trades"
    if rp.equity is not None:
        pos, eq = curves_from_trades(ohlc[2], tr)
        bad = np.nonzero(rp.pos[i, :bars] != pos)[0]
        assert not len(bad), f"{where}: pos differs first at bar {bad[:1]}"
        bad = np.nonzero(rp.equity[i, :bars] != eq)[0]
        assert not len(bad), f"{where}: equity differs first at bar {bad[:1]}"
        assert not rp.pos[i, bars:].any() and not rp.equity[i, bars:].any(), f"{where}: curve rows not zero past the bars"
    return s, tr


# ------------------------------------------------------------------------------------- edges
EDGE_BARS = (1, 2, 3, 63, 64, 65, 128, 129, 1000)
EDGE_IDS = (907, 12, 500, 3, 77, 2_000_000, 41, 8, 650)
# windows below 64, between 64 and 1,000, and above 1,000 (longer than every series)
EDGE_GRIDS = {
    "sma": lambda: D.Grid.sma([3, 70, 1200], [5, 100, 300, 2000], annualization=98280),
    "ema_ols": lambda: D.Grid.ema_ols([5, 80, 1500], [4, 64, 200, 1100], band_bps=5),
    "boll": lambda: D.Grid.boll([5, 64, 150, 1200], [2, 3, 4], [30], [60], k_den=2),
}


@functools.lru_cache(None)
def _edge_series():
    return [gen_hlc(0xED6E, i, b, 1) for i, b in zip(EDGE_IDS, EDGE_BARS)]


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_edges_every_lane_bit_exact(strategy):
    grid = EDGE_GRIDS[strategy]()
    assert grid.n_params == 12
    series = _edge_series()
    lanes = [(i, p) for i in EDGE_IDS for p in range(grid.n_params)]
    with D.Engine(grid) as e:
        _load(e, strategy, series, EDGE_IDS)
        rp = e.replay(lanes, trade_cap=CAP, curves=True)          # no run() before it
    assert rp.equity.shape == rp.pos.shape == (len(lanes), 1000)
    assert rp.trades.shape == (len(lanes), CAP) and rp.equity.dtype == np.int64 and rp.pos.dtype == np.int8
    traded = 0
    for i, (sym, p) in enumerate(lanes):
        k = EDGE_IDS.index(sym)
        s, _ = _check_lane(rp, i, strategy, grid, p, series[k], f"{strategy} sym {sym} ({EDGE_BARS[k]} bars) {grid.param(p)}")
        traded += int(s["n_trades"])
    assert traded >= 100


# --------------------------------------------------------------------- equal to the product
PRODUCT = {
    "config2": (D.config2_grid, 64, 2520, D.BT_DAILY),
    "config3": (D.config3_grid, 16, 6000, D.BT_MINUTE),
    "config4": (D.config4_grid, 16, 6000, D.BT_MINUTE),
}


@pytest.mark.parametrize("name", list(PRODUCT))
def test_replay_of_the_topk_equals_the_product(name):
    mk, n_sym, bars, freq = PRODUCT[name]
    grid = mk()
    with D.Engine(grid, topk=32) as e:
        e.load_synthetic(0xD1CE, 1000, n_sym, bars, freq)
        e.run()
        before = (e.summaries().copy(), e.read_topk().copy(), e.stats(), e.last_segments(with_refixed=True))
        top = before[1]
        assert len(top) == 32
        rp = e.replay(top)
        after = (e.summaries().copy(), e.read_topk().copy(), e.stats(), e.last_segments(with_refixed=True))
    assert rp.trades is None and rp.equity is None and rp.pos is None
    assert (rp.n_bars == bars).all()
    for i, rec in enumerate(top):
        where = f"{name} top {i} sym {rec['sym']} param {rec['param']}"
        got = rp.summaries[i]
        assert np.float64(got["sharpe"]).view(np.uint64) == np.float64(rec["sharpe"]).view(np.uint64), where
        assert int(got["pnl"]) == int(rec["pnl"]), where
        s, p = int(rec["sym"]) - 1000, int(rec["param"])
        compare_summaries(rp.summaries[i:i + 1], before[0][s:s + 1, p], lambda _: where)
        assert got.tobytes() == before[0][s, p].tobytes(), where
    assert before[0].tobytes() == after[0].tobytes()
    assert before[1].tobytes() == after[1].tobytes()
    assert before[2] == after[2] and before[3] == after[3]


# ------------------------------------------------------------------------------ cap and order
def test_trade_cap_and_request_order():
    grid = D.Grid.sma([3, 5], [20, 31], annualization=98280)
    n_sym, bars, cap = 3, 6000, 2
    series = [gen_hlc(0x5EED, 40 + s, bars, 1) for s in range(n_sym)]
    lanes = [(40 + s, p) for s in range(n_sym) for p in range(grid.n_params)]
    mixed = lanes[::-1] + [lanes[0], lanes[0], lanes[5]]
    with D.Engine(grid) as e:
        e.load_synthetic(0x5EED, 40, n_sym, bars, D.BT_MINUTE)
        rp = e.replay(lanes, trade_cap=cap)
        rm = e.replay(mixed, trade_cap=cap, curves=True)
        single = {ln: e.replay([ln], trade_cap=cap, curves=True) for ln in lanes}
    assert rp.trades.shape == (len(lanes), cap)
    many = 0
    for i, (sym, p) in enumerate(lanes):
        # first two trades exact, n_trades and the hash cover every trade
        s, _ = _check_lane(rp, i, "sma", grid, p, series[sym - 40], f"cap {cap} sym {sym} {grid.param(p)}", cap=cap)
        many += int(s["n_trades"]) > cap
    assert 2 * many >= len(lanes), "too few lanes exceed the cap"
    assert rm.lanes.tolist() == [tuple(x) for x in mixed]
    for i, ln in enumerate(mixed):
        one = single[ln]
        where = f"request {i} {ln}"
        assert rm.summaries[i].tobytes() == one.summaries[0].tobytes(), where
        assert rm.trades[i].tobytes() == one.trades[0].tobytes(), where
        assert rm.n_bars[i] == one.n_bars[0]
        assert np.array_equal(rm.equity[i], one.equity[0]) and np.array_equal(rm.pos[i], one.pos[0]), where
        assert rm.summaries[i].tobytes() == rp.summaries[lanes.index(ln)].tobytes(), where


# -------------------------------------------------------------------- many tiles and carries
LONG_BARS = 100_000
LONG_GRIDS = {
    "sma": lambda: D.Grid.sma([5, 150], [40, 3000], annualization=98280),
    "ema_ols": lambda: D.Grid.ema_ols([10, 390], [15, 1560], band_bps=10),
    # params 1 and 3 stop out at 1 bp, which a 1-min bar nearly always touches: exits at entry + 1
    "boll": lambda: D.Grid.boll([20, 240], [3, 5], [50, 1], [100], k_den=2),
}
LONG_PARAMS = (0, 1, 3)


@functools.lru_cache(None)
def _long_series():
    return gen_hlc(0x10C6, 5, LONG_BARS, 1)


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_many_tiles_and_carries(strategy):
    grid = LONG_GRIDS[strategy]()
    ohlc = _long_series()
    lanes = [(5, p) for p in LONG_PARAMS]
    with D.Engine(grid) as e:
        _load(e, strategy, [ohlc], [5])
        rp = e.replay(lanes, trade_cap=CAP, curves=True)
    assert rp.equity.shape == (3, LONG_BARS)
    for i, (_, p) in enumerate(lanes):
        s, tr = _check_lane(rp, i, strategy, grid, p, ohlc, f"{strategy} 100k {grid.param(p)}")
        assert int(s["n_trades"]) >= 20
        assert int(rp.equity[i, -1]) == int(s["pnl"])
        if strategy == "boll" and i == 1:
            # the walk has entries in a tile's last lane that exit on the next tile's first bar,
            # and exits in lane 0 and lane 63
            e_, x_ = tr["entry_bar"].astype(np.int64), tr["exit_bar"].astype(np.int64)
            assert ((e_ % 64 == 63) & (x_ == e_ + 1)).any() and (x_ % 64 == 0).any() and (x_ % 64 == 63).any()


# ---------------------------------------------------------- limits of the exactness argument
def _ceiling_series(bars=300):
    """Closes in [2^31 - 2^21, 2^31 - 2^20] (a reflected walk), o_t = c_(t-1), h >= max(o, c),
    l <= min(o, c): 64 squares of such closes sum past 2^63."""
    rng = np.random.default_rng(20261019)
    lo_, hi_ = 2**31 - 2**21, 2**31 - 2**20
    span = hi_ - lo_
    x = np.mod(span // 2 + np.cumsum(rng.integers(-150_000, 150_001, bars)), 2 * span)
    c = lo_ + np.where(x > span, 2 * span - x, x)
    o = np.concatenate([c[:1], c[:-1]])
    h = np.minimum(np.maximum(o, c) + rng.integers(0, 60_000, bars), 2**31 - 1)
    l = np.minimum(o, c) - rng.integers(0, 60_000, bars)
    return tuple(np.ascontiguousarray(v, np.int32) for v in (h, l, c))


def test_bollinger_squares_pass_int64_in_one_tile():
    h, l, c = _ceiling_series()
    c64 = c.astype(np.int64)
    assert c64.min() >= 2**31 - 2**21 and c64.max() <= 2**31 - 2**20 and len(c) == 300
    assert (h >= np.maximum(c64, np.concatenate([c64[:1], c64[:-1]]))).all()
    assert (l <= np.minimum(c64, np.concatenate([c64[:1], c64[:-1]]))).all()
    assert sum(int(v) ** 2 for v in c64[:64]) > 2**63
    # 1 bp is 214,748 ticks here: stops of 1-2 bp lie inside a bar's range
    grid = D.Grid.boll([64, 240], [1, 2], [1], [1, 2], k_den=2)
    lanes = [(0, p) for p in range(grid.n_params)]
    with D.Engine(grid) as e:
        _load(e, "boll", [(h, l, c)])
        rp = e.replay(lanes, trade_cap=CAP, curves=True)
    total = {64: 0, 240: 0}
    for i, (_, p) in enumerate(lanes):
        s, _ = _check_lane(rp, i, "boll", grid, p, (h, l, c), f"ceiling {grid.param(p)}")
        total[grid.param(p)["w"]] += int(s["n_trades"])
    assert total[64] >= 4 and total[240] >= 1, total


LONGEST = {
    "sma": lambda: D.Grid.sma([5, 600], [4096, 16192], annualization=98280),
    "ema_ols": lambda: D.Grid.ema_ols([10], [8512], band_bps=0),
    "boll": lambda: D.Grid.boll([20, 4608], [2, 3], [1], [2], k_den=2),
}


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_longest_accepted_windows(strategy):
    grid = LONGEST[strategy]()
    ohlc = gen_hlc(0x70BE, 9, 20_000, 1)
    lanes = [(0, p) for p in range(grid.n_params)]
    with D.Engine(grid) as e:
        _load(e, strategy, [ohlc])
        rp = e.replay(lanes, trade_cap=CAP, curves=True)
    for i, (_, p) in enumerate(lanes):
        s, _ = _check_lane(rp, i, strategy, grid, p, ohlc, f"longest {strategy} {grid.param(p)}")
        assert int(s["n_trades"]) >= 1, grid.param(p)


# ---------------------------------------------------------------------------------- refusals
def test_refusals_name_the_value_and_leave_the_engine_usable():
    grid = D.Grid.sma([3, 5], [20, 31], annualization=98280)
    ids, bars = (907, 12, 500), (200, 129, 64)
    series = [gen_hlc(0xBAD, i, b, 1) for i, b in zip(ids, bars)]
    P = grid.n_params

    def still_good(e):
        rp = e.replay([(12, 1), (907, 3)], trade_cap=CAP, curves=True)
        _check_lane(rp, 0, "sma", grid, 1, series[1], "after a refusal (12, 1)")
        _check_lane(rp, 1, "sma", grid, 3, series[0], "after a refusal (907, 3)")

    with D.Engine(grid) as e:
        with pytest.raises(D.BtError, match="no dataset"):
            e.replay([(907, 0)])
        _load(e, "sma", series, ids)
        still_good(e)
        for lanes, kw, named in (
            ([(907, 0), (999, 0)], {}, "999"),
            ([(907, P)], {}, rf"param {P} "),
            ([(907, -1)], {}, "param -1 "),
            ([(907, 0)] * (D.REPLAY_MAX + 1), {}, str(D.REPLAY_MAX + 1)),
            ([(907, 0)] * (D.REPLAY_MAX + 1), {"curves": True}, str(D.REPLAY_MAX + 1)),
            ([(907, 0)], {"trade_cap": -7}, "-7"),
        ):
            with pytest.raises(D.BtError, match=named):
                e.replay(lanes, **kw)
            still_good(e)
        # the raw binding: curves with a short stride; trades and trade_cap that disagree
        f = E.sym("bt_replay")
        req = D.as_lanes([(12, 0), (907, 0)])
        summ = np.zeros(2, D.SUMMARY_DTYPE)
        eq = np.zeros((2, 200), np.int64)
        tr = np.zeros((2, 4), D.TRADE_DTYPE)
        for args, named in (
            ((0, None, eq.ctypes.data, None, 199), "stride = 199 .*200 bars"),
            ((0, None, None, eq.ctypes.data, 0), "stride = 0 "),
            ((0, tr.ctypes.data, None, None, 0), "trade_cap = 0"),
            ((4, None, None, None, 0), "trade_cap = 4 "),
        ):
            cap, trp, eqp, posp, stride = args
            assert f(e._h, 2, req.ctypes.data, cap, summ.ctypes.data, None, trp, eqp, posp, stride) == -1
            msg = D.lib().bt_last_error().decode()
            assert re.search(named, msg), msg
            still_good(e)
        assert f(e._h, 2, req.ctypes.data, 0, summ.ctypes.data, None, None, eq.ctypes.data, None, 200) == 2
        # nothing requested
        for kw in ({}, {"trade_cap": 3, "curves": True}):
            rp = e.replay([], **kw)
            assert len(rp.lanes) == len(rp.summaries) == len(rp.n_bars) == 0
            assert rp.summaries.dtype == D.SUMMARY_DTYPE
            if kw:
                assert rp.trades.shape == (0, 3) and rp.equity.shape == (0, 0) and rp.pos.shape == (0, 0)
        still_good(e)


# --------------------------------------------------------------------------- bounded staging
def test_curves_of_1024_lanes_pass_through_bounded_staging():
    """1,024 x 100,000 bars of equity and position are 922 MB of host output, 3.6 times the
    device staging budget: the call succeeds in chunks and every row is the first one."""
    grid = LONG_GRIDS["sma"]()
    ohlc = _long_series()
    n = 1024
    with D.Engine(grid) as e:
        _load(e, "sma", [ohlc], [5])
        rp = e.replay([(5, 1)] * n, curves=True)
    assert rp.equity.shape == rp.pos.shape == (n, LONG_BARS)
    assert rp.equity.nbytes + rp.pos.nbytes > 900e6
    _check_lane(rp, 0, "sma", grid, 1, ohlc, "row 0 of 1,024")
    assert (rp.equity == rp.equity[0]).all() and (rp.pos == rp.pos[0]).all()
    assert (rp.summaries == rp.summaries[0]).all() and (rp.n_bars == LONG_BARS).all()
