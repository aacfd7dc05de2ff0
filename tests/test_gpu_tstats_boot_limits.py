"""bt_trade_stats and bt_bootstrap (k_tstats.hip, k_boot.hip) on the limit families B, C and D of
tests/limit_cases.py, which tests/test_gpu_walk_limits.py feeds to the other lane kernels (family A
runs in tests/test_gpu_tradestats.py and tests/test_gpu_bootstrap.py): exact Bollinger z ties, one
row of 2^22 bars at ceiling prices (65,536 tiles: the int32 counters mdd_bar, peak_bar, peak_at,
uw_run and hold_sum carried the whole way, and a bootstrap window 65,407 tiles in whose row the
planner itself puts into the arena), and the longest windows.

References: the C oracle's complete trade lists (the family's own rows where they are complete,
replay_ref.oracle_lane with the lane's own count otherwise), the curves of replay_ref, and
tradestats_ref / bootstrap_ref; rows of more than 20,000 bars go through the vectorised
tradestats_ref.lane_stats_fast, curves_from_trades_fast and bootstrap_ref.increments_fast, which the
unmarked tests here hold to bt_trade_stats_host and to the loops. Every comparison is bytes. The
unmarked tests also prove from the references that the rows reach what they are there for.

Family C holds the only cases of any length; the times measured on an MI355X are in the docstrings
of test_c_trade_stats_gpu and test_c_reality_check_gpu."""
import functools
import time

import numpy as np
import pytest

import bootstrap_ref as R
import dbx_amd as D
import tradestats_ref as T
from helpers import build_plan_driver, run_driver
from limit_cases import (B_GRIDS, B_TIES, C_ENGINES, CAP_B, CAP_D, D_ENGINES, MAXB, _b_case, _c_lane, _c_rows, _d_rows,
                         _hlc)
from replay_ref import curves_from_trades, curves_from_trades_fast, oracle_lane

OUTS = dict(per_lane=True, vmax=True, boot=True)
LONG = 20_000        # rows above this many bars take the vectorised references
BOOT = R.LIMITS      # B = 16, L = 100


def _load(e, strategy, series):
    """series: [(h, l, c)]; ids 0, 1, .."""
    if strategy == "boll":
        e.load_ohlc([s[2] for s in series], [s[0] for s in series], [s[1] for s in series])
    else:
        e.load_ohlc([s[2] for s in series])


def _lane_refs(c, trades):
    """(record, equity) of one lane from its closes and complete trade list."""
    if len(c) > LONG:
        eq = curves_from_trades_fast(c, trades)[1]
        return T.as_record(T.lane_stats_fast(trades, eq)), eq
    eq = curves_from_trades(c, trades)[1]
    return T.as_record(T.lane_stats(T.trade_tuples(trades), eq.tolist())), eq


def _increments(eq, frm, length):
    return R.increments_fast(eq, frm, length) if len(eq) > LONG else R.increments(eq, len(eq), frm, length)


def _host_record(trades, eq):
    return D.trade_stats_host(trades, eq)


# ----------------------------------------------------------------------------------------- C
C_T = 8200                           # above the 8,127 bars a row in LDS can hold
C_WINDOW = (MAXB - C_T, MAXB)        # it ends with the row; bar from - 1 lies in tile 65,407


@functools.lru_cache(None)
def _c_ref(name):
    """(recs 1 x P, the reality check of every lane in one group over C_WINDOW, the oracle's
    summaries) of one engine of family C; the curves of 32 MB each are not kept."""
    strategy, grid, hlc, rows = _c_rows(name)
    P = grid.n_params
    recs = np.zeros((1, P), D.TSTATS_DTYPE)
    d = []
    for p in range(P):
        summ, tr = _c_lane(name, p)
        assert int(summ["n_trades"]) == len(tr) == int(rows[p]["n_trades"]), (name, p)
        recs[0, p], eq = _lane_refs(hlc[2], tr)
        d.append(_increments(eq, C_WINDOW[0], C_T))
    recs.setflags(write=False)
    return recs, R.reality_check(d, [0, P], BOOT.B, BOOT.L, BOOT.seed), rows


@pytest.mark.parametrize("name", list(C_ENGINES))
def test_c_references_reach_the_long_counters(name):
    """From the references alone: drawdown bars past 2^21, a run under water of more than 65,536
    bars (more than a 16-bit counter holds, and more than 1,024 tiles), hold_sum the oracle's
    exposure; the vectorised record is bt_trade_stats_host's on every lane; and the planner puts the
    window's row into the arena by itself."""
    strategy, grid, hlc, rows = _c_rows(name)
    recs, boot, _ = _c_ref(name)
    P = grid.n_params
    assert recs.shape == (1, P) and len(hlc[2]) == MAXB == 1 << 22
    r = recs[0]
    assert (r["mdd_bar"] > 2**21).any() and (r["peak_bar"] > 2**21).any(), (r["mdd_bar"], r["peak_bar"])
    assert (r["max_underwater"] > 65536).any() and (r["underwater_bars"] > 2**21).any(), r["max_underwater"]
    assert (r["hold_sum"] > 2**20).any() and (r["n_bars"] == MAXB).all()
    for p in range(P):
        o = rows[p]
        assert int(r[p]["hold_sum"]) == int(o["exposure"]) and int(r[p]["n_trades"]) == int(o["n_trades"]) >= 1000
        assert int(r[p]["mdd"]) == int(o["mdd"]) and int(r[p]["hash"]) == int(o["hash"])
        assert int(r[p]["gross_win"]) - int(r[p]["gross_loss"]) == int(o["pnl"])
    p = int(np.argmax(r["max_underwater"]))      # the host code on the lane with the longest run
    _, tr = _c_lane(name, p)
    assert _host_record(tr, curves_from_trades_fast(hlc[2], tr)[1]).tobytes() == r[p].tobytes(), (name, p)
    # the window: T bars that end with the row, 65,407 tiles in, and a reference that moves
    frm, to = C_WINDOW
    assert to == MAXB and to - frm == C_T > 8127 and (frm - 1) // 64 == 65407
    assert boot.lanes["sum"].any() and len(set(boot.vmax[0].tolist())) > 1
    exe = build_plan_driver("boot_plan_driver")
    pl = run_driver(exe, P, 1, C_T, BOOT.B, BOOT.L, 1, 0, 1, 256, 0, 0)     # list mode, boot asked for, no row request
    assert pl["row_mode"] == 2 and pl["chunks"] == 1 and pl["lds_bytes"] == 512
    assert run_driver(exe, P, 1, 8127, BOOT.B, BOOT.L, 1, 0, 1, 256, 0, 0)["row_mode"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(C_ENGINES))
def test_c_trade_stats_gpu(name):
    """tstats_walk_kernel over 65,536 tiles, every lane in one call, records and aggregate.
    Measured on an MI355X with the engine and the load: 0.16 s (SMA, 6 lanes), 0.40 s (EMA+OLS, 4),
    0.41 s (the (10, 8512) lane), 0.42 s (Bollinger, 8), against 0.14 to 0.37 s of wf_walk_kernel
    over the same tiles (test_gpu_walk_limits.test_c_single_fold_gpu). As pytest reports the cases,
    with the references built once per process (oracle lanes, numpy curves, the vectorised record,
    the bootstrap's Python-int plan): 0.87 s, 1.02 s, 0.57 s and 1.61 s."""
    strategy, grid, hlc, _ = _c_rows(name)
    recs, _, _ = _c_ref(name)
    t0 = time.perf_counter()
    with D.Engine(grid) as e:
        _load(e, strategy, [hlc])
        ts = e.trade_stats(params=True)
    print(f"C {name}: trade_stats of {grid.n_params} lanes with its load {time.perf_counter() - t0:.2f} s")
    assert ts.lanes.shape == recs.shape == (1, grid.n_params)
    T.assert_same(ts.lanes, recs, f"C {name}: records")
    T.assert_same(ts.params, T.aggregate(recs), f"C {name}: aggregate")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(C_ENGINES))
def test_c_reality_check_gpu(name):
    """boot_kernel on the arena path by the planner's own choice: every lane walked through 65,536
    tiles, the 8,200 bars before the row's end resampled 16 times.
    Measured on an MI355X with the engine and the load: 0.08 s (SMA, 6 lanes), 0.25 s (EMA+OLS, 4),
    0.26 s (the (10, 8512) lane), 0.30 s (Bollinger, 8), which is what pytest reports: the reference
    is test_c_trade_stats_gpu's."""
    strategy, grid, hlc, _ = _c_rows(name)
    _, want, _ = _c_ref(name)
    lanes = [(0, p) for p in range(grid.n_params)]
    t0 = time.perf_counter()
    with D.Engine(grid) as e:
        _load(e, strategy, [hlc])
        got = e.reality_check(lanes, resamples=BOOT.B, block=BOOT.L, seed=BOOT.seed, window=C_WINDOW, **OUTS)
    print(f"C {name}: reality_check of {grid.n_params} lanes with its load {time.perf_counter() - t0:.2f} s")
    assert got.lanes.shape == (grid.n_params,)
    R.assert_same(got, want, f"C {name}: window {C_WINDOW}")


# ------------------------------------------------------------------------------------ B and D
def _b_tie_bar(tie):
    """The outlier bar of the fourth repetition, an untouched one (an exact tie)."""
    w = B_TIES[tie][0]
    return 3 * 6 + 5 if tie == "w6" else 3 * (w + 3) + w + 2


def _bd_rows(family, name):
    """(strategy, grid, series (c, h, l), oracle rows, the cap of those rows' trade lists)."""
    if family == "B":
        grid, series, oracle = _b_case(name)
        return "boll", grid, series, oracle, CAP_B
    strategy, grid, series, oracle = _d_rows(name)
    return strategy, grid, series, oracle, CAP_D


BD_CASES = [("B", n) for n in B_GRIDS] + [("D", n) for n in D_ENGINES]


@functools.lru_cache(None)
def _bd_ref(family, name):
    """(recs S x P, the bootstrap window or None for the whole row, the reality check of every lane
    in one group, the number of lanes whose trade list is the family's own, the number taken again
    from oracle_lane with the lane's own count)."""
    strategy, grid, series, oracle, cap = _bd_rows(family, name)
    hlc = _hlc(series)
    S, P = len(hlc), grid.n_params
    longest = max(len(c) for c, _, _ in series)
    window = None
    if longest > 100_000:            # w3970: a few thousand bars around an exact tie
        t = _b_tie_bar(B_GRIDS[name][0])
        window = (t - 2000, t + 2000)
    frm, length = window[0] if window else 0, window[1] - window[0] if window else longest
    recs = np.zeros((S, P), D.TSTATS_DTYPE)
    d, own, again = [], 0, 0
    for s, ohlc in enumerate(hlc):
        summs, lists = oracle[s]
        for p in range(P):
            n = int(summs[p]["n_trades"])
            if n <= cap:
                tr = lists[p]
                own += 1
            else:
                summ, tr = oracle_lane(strategy, grid, p, ohlc, cap=n)
                assert int(summ["n_trades"]) == n
                again += 1
            assert (0 if tr is None else len(tr)) == n, (family, name, s, p)
            recs[s, p], eq = _lane_refs(ohlc[2], tr)
            d.append(_increments(eq, frm, length))
    assert own + again == S * P == len(d), "every lane has a reference"
    recs.setflags(write=False)
    return recs, window, R.reality_check(d, [0, S * P], BOOT.B, BOOT.L, BOOT.seed), own, again


@pytest.mark.parametrize("family,name", BD_CASES)
def test_b_and_d_references_are_complete_and_the_host_code_s(family, name):
    """Every lane's reference comes from a complete trade list; the record is bt_trade_stats_host's
    (for the rows above 20,000 bars this holds the vectorised reference to the host code); the
    identities with the oracle's summaries; and what the family is there for is in the records."""
    strategy, grid, series, oracle, cap = _bd_rows(family, name)
    recs, window, boot, own, again = _bd_ref(family, name)
    S, P = recs.shape
    assert (S, P) == (len(series), grid.n_params) and own + again == S * P
    assert int(recs["n_trades"].sum()) >= 30 and boot.lanes["sum"].any()
    for s, (c, _, _) in enumerate(series):
        for p in range(P):
            o, r = oracle[s][0][p], recs[s, p]
            assert (int(r["n_trades"]), int(r["mdd"]), int(r["hash"])) == (int(o["n_trades"]), int(o["mdd"]), int(o["hash"]))
            assert int(r["gross_win"]) - int(r["gross_loss"]) == int(o["pnl"]) and int(r["hold_sum"]) == int(o["exposure"])
            assert int(r["n_bars"]) == len(c)
    # the host code on the first and the last lane (every lane of the long rows costs seconds)
    hlc = _hlc(series)
    for s, p in ((0, 0), (S - 1, P - 1)):
        n = int(oracle[s][0][p]["n_trades"])
        tr = oracle[s][1][p] if n <= cap else oracle_lane(strategy, grid, p, hlc[s], cap=n)[1]
        eq = (curves_from_trades_fast if len(hlc[s][2]) > LONG else curves_from_trades)(hlc[s][2], tr)[1]
        assert _host_record(tr, eq).tobytes() == recs[s, p].tobytes(), (family, name, s, p)
    longest = max(len(c) for c, _, _ in series)
    if window is None:
        assert longest <= 100_000
    else:                            # the tie bar lies inside the window, and lanes trade inside it
        t = _b_tie_bar(B_GRIDS[name][0])
        assert name == "w3970" and longest == 381_408 and window[0] < t < window[1] and window[1] - window[0] == 4000
    if family == "D":                # windows past the LDS row limit: the planner's arena path again
        assert longest > 8127 and again == 0


def test_the_fast_increments_are_the_loop_s():
    """bootstrap_ref.increments_fast against increments on curves of family B: windows from bar 0,
    inside the row, across its end and past it."""
    recs, _, _, _, _ = _bd_ref("B", "w5")
    grid, series, oracle = _b_case("w5")
    checked = 0
    for s, (c, _, _) in enumerate(series):
        for p in range(grid.n_params):
            eq = curves_from_trades(c, oracle[s][1][p])[1]
            for frm, length in ((0, len(c)), (0, 1), (1, 64), (100, 300), (len(c) - 10, 40), (len(c), 5), (len(c) + 3, 5)):
                assert R.increments_fast(eq, frm, length) == R.increments(eq, len(eq), frm, length), (s, p, frm, length)
                checked += 1
    assert checked == 2 * grid.n_params * 7 and recs["n_trades"].sum() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("family,name", BD_CASES)
def test_b_and_d_gpu(family, name):
    """trade_stats on every lane and reality_check with all lanes in one group over the whole row
    (w3970: 4,000 bars around a tie bar). Measured on an MI355X, as pytest reports the cases with
    their references: 0.09 to 0.11 s (D: sma, sma_wide, boll), every other case below 0.07 s."""
    strategy, grid, series, _, _ = _bd_rows(family, name)
    recs, window, want, _, _ = _bd_ref(family, name)
    hlc = _hlc(series)
    S, P = recs.shape
    lanes = [(s, p) for s in range(S) for p in range(P)]
    with D.Engine(grid) as e:
        _load(e, strategy, hlc)
        ts = e.trade_stats(params=True)
        rc = e.reality_check(lanes, resamples=BOOT.B, block=BOOT.L, seed=BOOT.seed, window=window, **OUTS)
    where = f"{family} {name}"
    assert ts.lanes.shape == (S, P) and rc.lanes.shape == (S * P,), f"{where}: every lane"
    T.assert_same(ts.lanes, recs, f"{where}: records")
    T.assert_same(ts.params, T.aggregate(recs), f"{where}: aggregate")
    R.assert_same(rc, want, f"{where}: reality check, window {window}")
