"""The lane kernels (walk_tile.h under k_replay.hip, k_walkfwd.hip, k_portfolio.hip, k_gram.hip) at
the limits of their own exactness arguments. walk_tile.h is a second device implementation of
docs/oracle_spec.md §4/§5 with one carried value per window sum and no prefix ring; it rests on
range arguments the sweep kernels do not share, each written as a comment:

* the OLS numerator from S and U = sum k c_k with ABSOLUTE k in uint64, "mod 2^64";
* "|q|, q2 <= 2^56: a tile's partial sums fit int64", followed by int128 running sums (k_replay.hip,
  and under a fold mask k_walkfwd.hip);
* the Bollinger z test as plain signed int128, D D kd2 > kn2 Q, without an fp64 bracket;
* cA, cB and the int128 cSc2 advanced by per-tile differences over up to 65,536 tiles.

The inputs are the four families of tests/limit_cases.py (tests/test_gpu_exact_limits.py feeds them
to the sweep kernels): A extreme returns, B exact z ties, C the maximum length at ceiling prices,
D the longest windows at ceiling prices. References: the C oracle's lanes (replay_ref.oracle_lane)
with the curves rebuilt from their trade lists, walkfwd_ref.ref_folds, portfolio_ref.portfolio and
gram_ref.covariance; every comparison is bytes, doubles by bits. The unmarked tests prove from the
references alone that the inputs reach the shapes named above.

Family C holds the only cases of any length; the times measured on an MI355X are in the docstrings
of test_c_replay_gpu and test_c_single_fold_gpu (0.14 s to 2.8 s a case).
"""
import functools
import re
import time

import numpy as np
import pytest

import dbx_amd as D
import gram_ref as G
import oracle_np as N
import orc_ffi as F
import portfolio_ref as PR
import walkfwd_ref as R
from helpers import compare_summary
from limit_cases import (B_GRIDS, B_TIES, C_ENGINES, C_GRIDS, CAP_A, CAP_B, CAP_D, D_ENGINES, D_SMA_WIDE, MAXB, REPS,
                         _a_case, _b_case, _c_lane, _c_rows, _d_rows, _hlc)
from replay_ref import curves_from_trades, curves_from_trades_fast

WHOLE = 2**31 - 1
STRATEGIES = ("sma", "ema_ols", "boll")   # family A's cases: ema_ols_128 adds nothing without stages
TRADE_FIELDS = ("entry_bar", "exit_bar", "side", "entry_px", "exit_px")


def _load(e, strategy, series):
    """series: [(h, l, c)]; ids 0, 1, .."""
    if strategy == "boll":
        e.load_ohlc([s[2] for s in series], [s[0] for s in series], [s[1] for s in series])
    else:
        e.load_ohlc([s[2] for s in series])


def _same_trades(row, want, n, where):
    """The first n records of a replay's trade row against the oracle's list, field by field as
    arrays; pad and the rest of the row are zero."""
    assert len(row) >= n and (n == 0 or len(want) >= n), f"{where}: {len(row)} trade slots, {n} trades"
    for f in TRADE_FIELDS if n else ():
        bad = np.nonzero(row[f][:n] != want[f][:n])[0]
        assert not len(bad), f"{where}: {f} differs first at trade {bad[0]}: {row[bad[0]]} vs {want[bad[0]]}"
    assert not row["pad"].any() and not row[n:].view(np.uint8).any(), f"{where}: trade row not zero past the trades"


def _same_curves(rp, i, pos, eq, where):
    bars = len(pos)
    bad = np.nonzero(rp.pos[i, :bars] != pos)[0]
    assert not len(bad), f"{where}: pos differs first at bar {bad[0]} ({len(bad)} bars)"
    bad = np.nonzero(rp.equity[i, :bars] != eq)[0]
    assert not len(bad), f"{where}: equity differs first at bar {bad[0]}: {rp.equity[i, bad[0]]} vs {eq[bad[0]]}"
    assert not rp.pos[i, bars:].any() and not rp.equity[i, bars:].any(), f"{where}: curve rows not zero past the bars"


def _fold_is_summary(f, o, bars, where):
    """walkforward_spec §3: with the single fold [0, B) every field is the whole-series figure.
    `o` is the C oracle's own summary with its int128 sums, so nothing here rests on Python."""
    for k in ("s1", "s2"):   # the exact sums first: a Sharpe equal by accident cannot hide a wrong one
        g, w = F.i128(f[k + "_lo"], f[k + "_hi"]), F.i128(o[k + "_lo"], o[k + "_hi"])
        assert g == w, f"{where}: {k} gpu={g} oracle={w}"
    for k in ("pnl", "n_trades", "exposure", "mdd"):
        assert int(f[k]) == int(o[k]), f"{where}: {k} gpu={f[k]} oracle={o[k]}"
    assert np.float64(f["sharpe"]).view(np.uint64) == np.float64(o["sharpe"]).view(np.uint64), \
        f"{where}: sharpe {float(f['sharpe'])!r} vs {float(o['sharpe'])!r}"
    assert (int(f["first_bar"]), int(f["n_bars"]), int(f["status"])) == (0, bars, 0), f"{where}: {f}"


def _accepted(grid):
    """bt_engine_create validates before it opens the device: an accepted grid gives an engine, or,
    on a machine without a GPU, the device error; a refused one its own message."""
    try:
        D.Engine(grid).close()
    except D.BtError as e:
        if not re.search("device|HIP", str(e)):
            raise
    return True


# ----------------------------------------------------------------------------------------- A
# 992 = 31 * 32: the crash bar (close 1 after 2^30 or 2^31 - 1) of both unshifted cycles, and 993
# that of the cycles shifted by one bar
A_CRASH = 992
A_EDGE = (0, 1, 63, 64, 65, 128, A_CRASH, A_CRASH + 1, 1000, 1200)
A_WINDOWS = ((0, WHOLE), (A_CRASH, WHOLE))
A_BARS = 1100   # the longest series of the family


@functools.lru_cache(None)
def _a_ref(name):
    """(strategy, grid, series (h, l, c), fold records of the edge layout, of the single fold,
    lanes[s][p] = (oracle summary, complete trade list), curves[s][p] = (pos, equity))."""
    strategy, grid, series, _ = _a_case(name)
    hlc = _hlc(series)
    edge, lanes = R.ref_folds(strategy, grid, hlc, A_EDGE)
    one, _ = R.ref_folds(strategy, grid, hlc, (0, WHOLE))
    curves = [[curves_from_trades(ohlc[2], lanes[s][p][1]) for p in range(grid.n_params)]
              for s, ohlc in enumerate(hlc)]
    return strategy, grid, hlc, edge, one, lanes, curves


def _a_entries(name):
    strategy, grid, hlc, _, _, _, curves = _a_ref(name)
    return [(s, p) for s in range(len(hlc)) for p in range(grid.n_params)]


@functools.lru_cache(None)
def _a_portfolio(name, window):
    _, grid, _, _, _, _, curves = _a_ref(name)
    return PR.portfolio([(curves[s][p][0].tolist(), curves[s][p][1].tolist(), *window) for s, p in _a_entries(name)],
                        A_BARS, grid.annualization)


@functools.lru_cache(None)
def _a_covariance(name, window):
    """gram_ref.covariance over every lane of the case. Lanes with the same curve (a Bollinger lane
    whose stops never fill beside its neighbour, a lane that never trades on two series) have the
    same row and column: the Python-int products run once per distinct curve and are copied out,
    gram[i][j] being a function of curves i and j alone."""
    _, _, _, _, _, _, curves = _a_ref(name)
    index, distinct, of = {}, [], []
    for s, p in _a_entries(name):
        eq = curves[s][p][1]
        k = (len(eq), eq.tobytes())
        if k not in index:
            index[k] = len(distinct)
            distinct.append(eq.tolist())
        of.append(index[k])
    g, sums, T = G.covariance(distinct, window)
    of = np.asarray(of)
    return g[np.ix_(of, of)], sums[of], T


def test_a_fast_curves_are_the_loop_s():
    """curves_from_trades_fast (difference arrays and prefix sums, family C's reference) against
    curves_from_trades on every lane of family A: flips at one bar, exits at entry + 1, trades that
    end at the last bar, lanes that never trade."""
    lanes = flips = 0
    for name in STRATEGIES:
        strategy, grid, hlc, _, _, rows, curves = _a_ref(name)
        for s, ohlc in enumerate(hlc):
            for p in range(grid.n_params):
                tr = rows[s][p][1]
                pos, eq = curves_from_trades_fast(ohlc[2], tr)
                want = curves[s][p]
                assert pos.dtype == want[0].dtype and eq.dtype == want[1].dtype
                assert np.array_equal(pos, want[0]) and np.array_equal(eq, want[1]), (name, s, grid.param(p))
                lanes += 1
                flips += int((tr["exit_bar"][:-1] == tr["entry_bar"][1:]).sum()) if len(tr) > 1 else 0
    assert lanes == 81 + 36 + 432 and flips >= 1000
    pos, eq = curves_from_trades_fast(np.arange(1, 6), None)
    assert not pos.any() and not eq.any() and len(pos) == len(eq) == 5


@pytest.mark.parametrize("name", STRATEGIES)
def test_a_reaches_the_wide_sums(name):
    strategy, grid, hlc, edge, one, rows, curves = _a_ref(name)
    # the edge layout cuts on a crash bar and on the bar after one
    c = [ohlc[2].astype(np.int64) for ohlc in hlc]
    assert any(x[A_CRASH] == 1 and x[A_CRASH - 1] >= 2**30 for x in c)
    assert any(x[A_CRASH + 1] == 1 and x[A_CRASH] >= 2**30 for x in c)
    assert max(len(x) for x in c) == A_BARS
    # fold cells whose sums pass one word
    cells = edge.reshape(-1)
    s2 = [F.i128(f["s2_lo"], f["s2_hi"]) for f in cells]
    s1 = [F.i128(f["s1_lo"], f["s1_hi"]) for f in cells]
    assert max(s2) >= 2**64 and max(abs(x) for x in s1) >= 2**64, (name, max(s2), max(abs(x) for x in s1))
    assert min(s2) >= 0
    # the covariance call's domain and size
    n = len(hlc) * grid.n_params
    assert n == len(_a_entries(name)) <= D.COV_MAX == 2048
    for s in range(len(hlc)):
        for p in range(grid.n_params):
            assert int(rows[s][p][0]["n_trades"]) <= CAP_A
            d = np.diff(curves[s][p][1], prepend=0)
            assert int(np.abs(d).max()) < 2**31, (name, s, grid.param(p))
    # the book of every lane: its sum of squares passes one word where a lane's move is a whole
    # price (the EMA+OLS lanes hold through moves of at most 2^24 ticks)
    for w in A_WINDOWS:
        assert (int(_a_portfolio(name, w)[4]["s2_hi"]) != 0) == (name != "ema_ols"), (name, w)
    # the single fold of the Python reference is the oracle's own summary
    _, _, _, oracle = _a_case(name)
    for s, (orc, _) in enumerate(oracle):
        for p in range(grid.n_params):
            _fold_is_summary(one[s, p, 0], orc[p], len(c[s]), f"A {name} reference series {s} {grid.param(p)}")


def test_a_sma_tile_sums_come_within_2_40_of_2_62():
    """"|q|, q2 <= 2^56: a tile's partial sums fit int64": the (1, 2) lane is in a position on every
    bar after the first, so a 64-bar tile's sum of q2 over held bars is 64 returns; on the tiles
    without a crash bar every one of them is 2^56."""
    strategy, grid, hlc, _, _, rows, curves = _a_ref("sma")
    p = next(p for p in range(grid.n_params) if grid.param(p) == {"f": 1, "s": 2})
    best = 0
    for s, ohlc in enumerate(hlc):
        q2 = np.array(N.fixed_returns(ohlc[2])[1], np.int64)    # each <= 2^56
        pos = curves[s][p][0]
        held = np.concatenate([[False], pos[:-1] != 0])
        assert int(held.sum()) == int(rows[s][p][0]["exposure"]) == len(pos) - 2
        for t0 in range(0, len(pos), 64):
            best = max(best, sum(int(x) for x in q2[t0:t0 + 64][held[t0:t0 + 64]]))
    assert 2**62 - 2**40 <= best <= 2**62, best


@pytest.mark.gpu
@pytest.mark.parametrize("name", STRATEGIES)
def test_a_replay_gpu(name):
    strategy, grid, hlc, _, _, rows, curves = _a_ref(name)
    lanes = _a_entries(name)
    with D.Engine(grid) as e:
        _load(e, strategy, hlc)
        rp = e.replay(lanes, trade_cap=CAP_A, curves=True)
    assert rp.equity.shape == rp.pos.shape == (len(lanes), A_BARS)
    for i, (s, p) in enumerate(lanes):
        where = f"A {name} series {s} {grid.param(p)}"
        summ, tr = rows[s][p]
        compare_summary(rp.summaries[i], summ, where)
        assert int(rp.n_bars[i]) == len(hlc[s][2]), where
        _same_trades(rp.trades[i], tr, int(summ["n_trades"]), where)
        _same_curves(rp, i, *curves[s][p], where)


@pytest.mark.gpu
@pytest.mark.parametrize("name", STRATEGIES)
def test_a_walk_forward_gpu(name):
    strategy, grid, hlc, edge, one, _, _ = _a_ref(name)
    _, _, _, oracle = _a_case(name)
    with D.Engine(grid) as e:
        _load(e, strategy, hlc)
        got_one = e.walk_forward((0, WHOLE), train=0, folds=True)
        got_edge = e.walk_forward(A_EDGE, train=1, folds=True)
    for s, (orc, _) in enumerate(oracle):
        for p in range(grid.n_params):
            _fold_is_summary(got_one.folds[s, p, 0], orc[p], len(hlc[s][2]), f"A {name} series {s} {grid.param(p)}")
    R.assert_same(got_one.folds, one, f"A {name} single fold")
    R.assert_same(got_edge.folds, edge, f"A {name} edge folds")


@pytest.mark.gpu
@pytest.mark.parametrize("name", STRATEGIES)
def test_a_portfolio_and_covariance_gpu(name):
    strategy, grid, hlc, _, _, _, _ = _a_ref(name)
    lanes = _a_entries(name)
    with D.Engine(grid) as e:
        _load(e, strategy, hlc)
        pf = {w: e.portfolio(lanes, windows=w) for w in A_WINDOWS}
        cv = {w: e.covariance(lanes, w) for w in A_WINDOWS}
    for w in A_WINDOWS:
        want = _a_portfolio(name, w)
        assert int(want[4]["n_lanes"]) == len(lanes) and int(want[4]["first_bar"]) == w[0]
        PR.assert_equal(pf[w], want, f"A {name} portfolio window {w}")
        G.assert_equal(cv[w], _a_covariance(name, w), f"A {name} covariance window {w}")


# ----------------------------------------------------------------------------------------- B
B_SHORT = [n for n in B_GRIDS if B_GRIDS[n][0] != "w3970"]


def _b_tie_bar(tie):
    """The outlier bar of the fourth repetition, an untouched one (an exact tie)."""
    w = B_TIES[tie][0]
    return 3 * 6 + 5 if tie == "w6" else 3 * (w + 3) + w + 2


@functools.lru_cache(None)
def _b_folds(name):
    """[(bounds, fold records)] of a short tie: the single fold, and cuts on a tie bar and after it."""
    grid, series, _ = _b_case(name)
    t = _b_tie_bar(B_GRIDS[name][0])
    bars = len(series[0][0])
    return [(b, R.ref_folds("boll", grid, _hlc(series), b)[0]) for b in ((0, WHOLE), (0, t, t + 1, bars))]


def test_b_operands_stay_below_2_127():
    """The z test is signed int128: over the w = 3970 series, at the family's largest k_num and
    k_den, max(D^2 kd^2, kn^2 Q) < 2^127 (Python ints), and past 2^110 as the sweep tests show."""
    w, K, kd, _ = B_TIES["w3970"]
    grid, series, _ = _b_case("w3970")
    kn = max(int(k) for k in grid.axes[1])
    assert kn == K * kd + 1 and w * kn < 2**32
    top = 0
    for c, _, _ in series:
        c = c.astype(np.int64)
        p1 = np.concatenate([[0], np.cumsum(c)])                       # < 2^50
        p2 = np.concatenate([[0], np.cumsum(c.astype(object) ** 2)])   # Python ints
        t = np.arange(w - 1, len(c))
        S1 = (p1[t + 1] - p1[t + 1 - w]).astype(object)
        Dv = w * c[t].astype(object) - S1
        Q = w * (p2[t + 1] - p2[t + 1 - w]) - S1 * S1
        assert min(Q) >= 0
        top = max(top, max(Dv * Dv) * kd * kd, kn * kn * max(Q))
    assert 2**110 < top < 2**127, top


@pytest.mark.parametrize("name", B_SHORT)
def test_b_fold_bounds_sit_on_an_exact_tie(name):
    """The bar the folds are cut on is an exact tie with D != 0 on both series, and the tied k does
    not trade there while the k below it does (the strict test)."""
    grid, series, oracle = _b_case(name)
    tie, offs, _, _, kd = B_GRIDS[name]
    w, K, kd0, _ = B_TIES[tie]
    kd = kd or kd0
    t = _b_tie_bar(tie)
    nlev = len(grid.axes[2]) * len(grid.axes[3])
    for i, (c, _, _) in enumerate(series):
        win = [int(x) for x in c[t - w + 1:t + 1]]
        Dv, Q = w * win[-1] - sum(win), w * sum(x * x for x in win) - sum(win) ** 2
        assert Dv != 0 and Dv * Dv * kd * kd == (K * kd) ** 2 * Q, (name, i, t)
        _, trs = oracle[i]
        below, tied = trs[offs.index(-1) * nlev], trs[offs.index(0) * nlev]
        assert (below["entry_bar"] == t).any() and not (tied["entry_bar"] == t).any(), (name, i, t)
    for bounds, folds in _b_folds(name):
        assert folds.shape == (2, grid.n_params, len(bounds) - 1) and folds["n_trades"].sum() >= REPS // 3


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(B_GRIDS))
def test_b_z_ties_gpu(name):
    grid, series, oracle = _b_case(name)
    hlc = _hlc(series)
    lanes = [(s, p) for s in range(len(hlc)) for p in range(grid.n_params)]
    with D.Engine(grid) as e:
        _load(e, "boll", hlc)
        rp = e.replay(lanes, trade_cap=CAP_B)
        wf = [e.walk_forward(b, train=0, folds=True) for b, _ in _b_folds(name)] if name in B_SHORT else []
    for i, (s, p) in enumerate(lanes):
        where = f"B {name} series {s} {grid.param(p)}"
        orc, trs = oracle[s]
        compare_summary(rp.summaries[i], orc[p], where)
        _same_trades(rp.trades[i], trs[p], min(int(orc[p]["n_trades"]), CAP_B), where)
    for got, (bounds, folds) in zip(wf, _b_folds(name) if wf else ()):
        R.assert_same(got.folds, folds, f"B {name} folds {bounds}")
        if len(bounds) == 2:
            for s, p in lanes:
                _fold_is_summary(got.folds[s, p, 0], oracle[s][0][p], len(hlc[s][2]), f"B {name} series {s} param {p}")


# ----------------------------------------------------------------------------------------- C
C_WRAP = 1_020_000   # U_t >= 2^64 from about this bar on at w = 8512


def test_c_window_sums_wrap_2_64():
    """With Python ints at a handful of bars: U_t = sum k c_k over the window and (t - w + 1) S_t,
    the two terms of the OLS numerator the walk subtracts mod 2^64."""
    strategy, grid, hlc, rows = _c_rows("ema_ols_8512")
    assert grid.param(0)["w"] == 8512 and grid.param(0)["n"] == 10 and grid.n_params == 1
    c = hlc[2].astype(np.int64)
    assert len(c) == MAXB

    def sums(t, w):
        k = range(t - w + 1, t + 1)
        win = c[t - w + 1:t + 1].tolist()
        return sum(a * b for a, b in zip(k, win)), sum(win)

    for t in (C_WRAP, 2**21, 2**22 - 1):
        U, S = sums(t, 8512)
        assert U >= 2**64 and (t - 8512 + 1) * S >= 2**64, (t, U, S)
    U, _ = sums(1_000_000, 8512)
    assert U < 2**64
    U, _ = sums(2**22 - 1, 1560)
    assert 2**63 <= U < 2**64 and 1560 in C_GRIDS["ema_ols"]().axes[1]
    # the lane is decided by wrapped sums on most of its trades
    summ, tr = _c_lane("ema_ols_8512", 0)
    assert len(tr) == int(summ["n_trades"]) == int(rows[0]["n_trades"])
    assert int((tr["entry_bar"] > C_WRAP).sum()) >= 100_000


@pytest.mark.parametrize("name", list(C_ENGINES))
def test_c_every_lane_trades(name):
    strategy, grid, hlc, rows = _c_rows(name)
    assert grid.n_params <= 8 and _accepted(grid)
    assert min(int(o["n_trades"]) for o in rows) >= 1000


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(C_ENGINES))
def test_c_replay_gpu(name):
    """Every lane with its whole trade list and both curves: 65,536 sequential tiles per lane, one
    call per lane since the trade cap is the lane's own trade count (3,893 to 460,745 trades).
    Measured on an MI355X, the replay calls (kernel, 36 MB of curves and the trades copied out) and
    beside them the lanes' oracle runs with the numpy curves: SMA 6 lanes 0.67 s + 0.22 s, EMA+OLS
    4 lanes 1.16 s + 0.17 s, the (10, 8512) lane 0.37 s + 0.05 s, Bollinger 8 lanes 2.18 s + 0.38 s;
    as pytest reports the cases with their comparisons: 1.15 s, 1.47 s, 0.46 s and 2.80 s. Every lane
    keeps its curves: no case comes near 5 s."""
    strategy, grid, hlc, rows = _c_rows(name)
    t_gpu = t_ref = 0.0
    with D.Engine(grid) as e:
        _load(e, strategy, [hlc])
        for p in range(grid.n_params):
            where = f"C {name} {grid.param(p)}"
            t0 = time.perf_counter()
            summ, tr = _c_lane(name, p)
            n = int(summ["n_trades"])
            assert n == len(tr) == int(rows[p]["n_trades"]), where
            pos, eq = curves_from_trades_fast(hlc[2], tr)
            t1 = time.perf_counter()
            rp = e.replay([(0, p)], trade_cap=n, curves=True)
            t2 = time.perf_counter()
            t_ref, t_gpu = t_ref + t1 - t0, t_gpu + t2 - t1
            compare_summary(rp.summaries[0], summ, where)
            assert int(rp.n_bars[0]) == MAXB and rp.trades.shape == (1, n) and rp.equity.shape == (1, MAXB), where
            _same_trades(rp.trades[0], tr, n, where)
            _same_curves(rp, 0, pos, eq, where)
            assert int(rp.equity[0, -1]) == int(summ["pnl"]), where
    print(f"C {name}: {grid.n_params} lanes, replay calls {t_gpu:.2f} s, oracle lanes and curves {t_ref:.2f} s")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(C_ENGINES))
def test_c_single_fold_gpu(name):
    """wf_walk_kernel over 65,536 tiles with the single fold (0, 2^22): the record is the oracle
    row, its int128 sums and every other field walkforward_spec §3 says coincides. Measured on an
    MI355X with the engine and the load: 0.14 s (SMA, 6 lanes), 0.32 s (EMA+OLS, 4), 0.33 s (the
    (10, 8512) lane), 0.37 s (Bollinger, 8): at most 5 to 6 us per tile, the load included."""
    strategy, grid, hlc, rows = _c_rows(name)
    t0 = time.perf_counter()
    with D.Engine(grid) as e:
        _load(e, strategy, [hlc])
        wf = e.walk_forward((0, MAXB), train=0, folds=True)
    print(f"C {name}: walk_forward of {grid.n_params} lanes with its load {time.perf_counter() - t0:.2f} s")
    assert wf.folds.shape == (1, grid.n_params, 1)
    for p in range(grid.n_params):
        _fold_is_summary(wf.folds[0, p, 0], rows[p], MAXB, f"C {name} {grid.param(p)}")


# ----------------------------------------------------------------------------------------- D
# limit_cases.D_ENGINES: D_GRIDS' own SMA lanes have f <= 600: F s stays below 600 * 2^31 * 16192 = 2^54.3. Two more lanes
# on the same series carry the F s = L f comparison to the top of its range: 2 F = L and 4 F = 3 L
# at products of 2^58 and 2^58.6 (the walk's comment bounds them by 2^59).
def test_d_sma_ties_at_the_top_of_the_product_range():
    """Decision bars of the flat series (0-3 ticks of noise under 2^31 - 2^20) with F s == L f
    exactly, the largest of them at a product >= 2^57; the tied bars change no position."""
    ties, top = {}, 0
    for name in ("sma", D_SMA_WIDE):
        _, grid, series, oracle = _d_rows(name)
        assert _accepted(grid)
        c = series[0][0].astype(np.int64)
        pre = np.concatenate([[0], np.cumsum(c)])
        for p in range(grid.n_params):
            f, s = grid.param(p)["f"], grid.param(p)["s"]
            t = np.arange(max(f, s) - 1, len(c) - 1)      # decision bars: warm .. B - 2
            Fs = (pre[t + 1] - pre[t + 1 - f]) * s        # < 2^59 in int64
            Lf = (pre[t + 1] - pre[t + 1 - s]) * f
            tied = Fs == Lf
            ties[f, s] = int(tied.sum())
            if tied.any():
                top = max(top, int(Fs[tied].max()))
                _, trs = oracle[0]
                assert not np.isin(trs[p]["entry_bar"], t[tied]).any(), (f, s)
            assert int(oracle[0][0][p]["n_trades"]) <= CAP_D
    assert ties[8096, 16192] >= 10 and ties[5, 20] >= 100, ties
    assert 2**57 <= top < 2**59, (top, ties)


@pytest.mark.gpu
@pytest.mark.parametrize("name", D_ENGINES)
def test_d_longest_windows_gpu(name):
    strategy, grid, series, oracle = _d_rows(name)
    hlc = _hlc(series)
    lanes = [(s, p) for s in range(len(hlc)) for p in range(grid.n_params)]
    with D.Engine(grid) as e:
        _load(e, strategy, hlc)
        rp = e.replay(lanes, trade_cap=CAP_D)
    for i, (s, p) in enumerate(lanes):
        where = f"D {name} series {s} {grid.param(p)}"
        orc, trs = oracle[s]
        n = int(orc[p]["n_trades"])
        assert n <= CAP_D, where
        compare_summary(rp.summaries[i], orc[p], where)
        _same_trades(rp.trades[i], trs[p], n, where)
