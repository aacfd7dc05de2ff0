"""The kernels at the limits their exactness arguments assume. Every GPU parity test compares
the HIP path with the C oracle bit for bit; these inputs sit where that equality rests on a range
argument written in a comment, each valid by docs/oracle_spec.md (1 <= c < 2^31,
|c_t - c_(t-1)| <= c_(t-1)):

A. |ret| = 1 on almost every bar (doubling cycles 1, 2, ..., 2^30): q2 = 2^56, so S1 and S2
   pass 64 bits within 1,100 bars (tile_common.h I96 carries, the segment records' hi words,
   the wide branch of internal.h i128_to_double on the device) and the SMA kernel's uint64
   return partials come within 2^30 of 2^63 over a 128-bar pair (k_sma.hip).
B. Bollinger z tests that are exactly tied, D^2 k_den^2 = k_num^2 Q with D != 0, or one tick
   from tied, at operands up to 2^112: the fp64 bracket of k_boll.hip cannot decide them and
   the int128 settle path does, also in the second pass of 8 thresholds and at the edge of
   window * k < 2^32.
C. One symbol of kMaxBars = 2^22 bars at prices within 2^21 of 2^31: the prefix of c ends
   within 0.1 % of 2^53, the bound under which the prefix rings are exact doubles.
D. The longest windows bt_engine_create accepts (docs/oracle_spec.md §7), at ceiling prices.

The unmarked tests prove on the CPU, with the two oracles and small models of the kernel's
rules, that the seeded inputs reach these shapes; the gpu tests compare every summary field,
the trades and (parity instantiation) the 128-bit sums S1, S2 with the C oracle. The inputs are
built in tests/limit_cases.py, which tests/test_gpu_walk_limits.py feeds to the lane kernels.
"""
import re

import numpy as np
import pytest

import dbx_amd as D
import oracle_np as N
import orc_ffi as F
from helpers import compare_summary, compare_trades, launch_plan, oracle_row
from limit_cases import (A_CASES, B_GRIDS, B_TIES, C_GRIDS, CAP_A, CAP_B, CAP_D, D_GRIDS, D_LIMITS, MAXB, REPS,
                         _a_case, _a_closes, _assert_valid, _b_case, _b_series, _c_case, _d_case, _i32, _wicks)

NP_FIELDS = (("n_trades", "n"), ("pnl", "pnl"), ("mdd", "mdd"), ("exposure", "exposure"), ("hash", "h"))


def _assert_np_equal(strategy, grid, ohlc, orc, where):
    """oracle_np.run (direct window formulas, Python ints) vs the C oracle's summaries."""
    c, h, lo = ohlc
    for p in range(grid.n_params):
        got, _ = N.run(strategy, (c, h, lo, c), grid.param(p), grid.annualization)
        for cf, nf in NP_FIELDS:
            assert int(orc[p][cf]) == got[nf], f"{where} {grid.param(p)}: {cf}"
        assert F.i128(orc[p]["s1_lo"], orc[p]["s1_hi"]) == got["s1"], f"{where} {grid.param(p)}: s1"
        assert F.i128(orc[p]["s2_lo"], orc[p]["s2_hi"]) == got["s2"], f"{where} {grid.param(p)}: s2"
        assert float(orc[p]["sharpe"]) == got["sharpe"], f"{where} {grid.param(p)}: sharpe"


def _gpu_check(strategy, grid, series, oracle, mode, cap, what):
    """One engine run of `series` against `oracle` (the rows of _oracle). mode: "parity" (trade
    lists and the 128-bit sums compared as well), 0 (release, automatic segmentation) or n >= 1
    (release, n segments per symbol)."""
    parity = mode == "parity"
    with D.Engine(grid, **(dict(parity=True, trade_cap=cap) if parity else {})) as e:
        if not parity:
            e.set_segments(mode)
        if strategy == "boll":
            e.load_ohlc([s[0] for s in series], [s[1] for s in series], [s[2] for s in series])
        else:
            e.load_ohlc([s[0] for s in series])
        e.run()
        if not parity and mode >= 1:
            assert e.last_segments() == mode
        got = e.summaries()
        sums, tr = (e.sums(), e.trades()) if parity else (None, None)
    for s, (orc, otr) in enumerate(oracle):
        for p in range(grid.n_params):
            where = f"{what} mode {mode} series {s} {grid.param(p)}"
            if parity:  # the exact sums first: a Sharpe equal by accident cannot hide a wrong one
                for k in ("s1", "s2"):
                    g = F.i128(sums[s, p][k + "_lo"], sums[s, p][k + "_hi"])
                    o = F.i128(orc[p][k + "_lo"], orc[p][k + "_hi"])
                    assert g == o, f"{where}: {k} gpu={g} oracle={o}"
            compare_summary(got[s, p], orc[p], where)
            if parity:
                compare_trades(tr[s, p], otr[p], min(int(orc[p]["n_trades"]), cap), where)


# ----------------------------------------------------------------------------------------- A
def test_a_cycles_are_valid_and_crash_on_every_tile_position():
    for long_series in (False, True):
        _assert_valid([_i32(c, *_wicks(c)) for c in _a_closes(long_series)])
    cl = _a_closes()
    assert [len(c) for c in cl[:4]] == [1025, 1024, 1000, 1100] and len(cl[0]) % 64 == 1 and len(cl[1]) % 128 == 0
    # the 32-bar cycle keeps its phase against the 128-bar pairs: the crash bar (close 1 after
    # 2^31 - 1) falls on a tile's first bar, mid-tile in both tiles of a pair, and on a last bar
    pos = [set(int(t) % 128 for t in np.nonzero(c[1:] == 1)[0] + 1) for c in cl[4:8]]
    assert pos[0] == {0, 32, 64, 96} and pos[1] == pos[2] == {1, 33, 65, 97} and pos[3] == {31, 63, 95, 127}
    # the 31-bar cycle drifts through every position
    assert set(int(t) % 128 for c in cl[:4] for t in np.nonzero(c[1:] == 1)[0] + 1) >= {0, 63, 64, 127}


@pytest.mark.parametrize("name", list(A_CASES))
def test_a_sums_pass_64_bits(name):
    strategy, grid, series, oracle = _a_case(name)
    held = wide2 = wide1 = 0
    for orc, _ in oracle:
        for o in orc:
            assert int(o["n_trades"]) <= CAP_A
            if int(o["exposure"]):
                held += 1
                wide2 += F.i128(o["s2_lo"], o["s2_hi"]) >= 2**64
                wide1 += abs(F.i128(o["s1_lo"], o["s1_hi"])) >= 2**64
    assert held and 2 * wide2 >= held and wide1 >= 1, (held, wide2, wide1)


def test_a_sma_partials_come_within_2_40_of_2_63():
    """The (1, 2) lane is in a position on every bar after the first (long after an up bar, short
    after a down bar), so its uint64 partial of q2 over a 128-bar pair of tiles is the plain sum."""
    best = 0
    for c in _a_closes():
        orc, _ = F.sma(c, 1, 2, 252)
        assert int(orc["exposure"]) == len(c) - 2     # flat only after bar 0 and after the last
        q2 = N.fixed_returns(c)[1]
        pairs = [sum(q2[t:t + 128]) for t in range(0, len(c) - 127, 128)]
        assert all(x < 2**63 for x in pairs)
        best = max(best, max(pairs))
    assert 2**63 - 2**40 <= best < 2**63, best


@pytest.mark.parametrize("name", list(A_CASES))
def test_a_oracles_agree(name):
    strategy, grid, series, oracle = _a_case(name)
    if name == "ema_ols_128":  # the short-window lanes ran above; here 1,560-bar ones (O(bars x window))
        grid = D.Grid.ema_ols([3, 40], [1560])
        oracle = [oracle_row(strategy, grid, (c, h, lo, c), grid.annualization) for c, h, lo in series]
    for i, ((orc, _), ohlc) in enumerate(zip(oracle, series)):
        _assert_np_equal(strategy, grid, ohlc, orc, f"A {name} series {i}")


def test_a_128_bar_stage_grid():
    assert launch_plan(A_CASES["ema_ols_128"][1]())["ts"] == 2
    assert launch_plan(A_CASES["ema_ols"][1]())["ts"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["parity", 1, 2, 3])
@pytest.mark.parametrize("name", list(A_CASES))
def test_a_extreme_returns_gpu(name, mode):
    strategy, grid, series, oracle = _a_case(name)
    _gpu_check(strategy, grid, series, oracle, mode, CAP_A, f"A {name}")


# ----------------------------------------------------------------------------------------- B
def _bracket(c, w, k_num, k_den):
    """The fp64 z test of k_boll.hip (boll flags, `S2d` ... `ztest`), the same operations in the
    same order in numpy float64, for every full window of `c`; then the exact integers of the
    windows it leaves undecided. Returns per undecided window with D != 0 the pair (L, R) =
    (D^2 k_den^2, k_num^2 Q) as Python ints, and max(L, R) over all windows."""
    c = np.asarray(c, np.int64)
    c2 = c * c
    pre = lambda x: np.concatenate([[0], np.cumsum(x)])
    p1, ph, pl = pre(c), pre(c2 >> 31), pre(c2 & 0x7FFFFFFF)
    assert p1[-1] < 2**53 and ph[-1] < 2**53 and pl[-1] < 2**53   # exact as doubles
    t = np.arange(w - 1, len(c))
    S1, H, L = (p[t + 1] - p[t + 1 - w] for p in (p1, ph, pl))
    S1d, dH, dL = S1.astype(np.float64), H.astype(np.float64), L.astype(np.float64)
    wlen = np.float64(w)
    Dd = wlen * c[t].astype(np.float64) - S1d
    S2d = dH * 2.0**31 + dL
    pd = wlen * S2d
    Qd = pd - S1d * S1d
    QH = (Qd + pd * 2.0**-48) * (1.0 + 2.0**-47)
    QL = (Qd - pd * 2.0**-48) * (1.0 - 2.0**-47)
    lh = (Dd * Dd) * np.float64(k_den * k_den)
    kn2 = np.float64(k_num * k_num)
    big = lh > kn2 * QH
    small = kn2 * QL > lh
    exact = lambda i: (w * int(c[t[i]]) - int(S1[i]), w * ((int(H[i]) << 31) + int(L[i])) - int(S1[i])**2)
    pairs = []
    for i in np.nonzero(~big & ~small)[0]:
        Dx, Qx = exact(i)
        if Dx:
            pairs.append((Dx * Dx * k_den * k_den, k_num * k_num * Qx))
    # the bracket is sound: what it decides, the integers decide the same way
    for i in np.concatenate([np.nonzero(big)[0][:50], np.nonzero(small)[0][:50]]):
        Dx, Qx = exact(i)
        assert (Dx * Dx * k_den * k_den > k_num * k_num * Qx) == bool(big[i])
    top = max(max(abs(Dd)) ** 2 * k_den * k_den, max(Qd) * k_num * k_num)
    return pairs, top


@pytest.mark.parametrize("tie", list(B_TIES))
def test_b_bracket_leaves_the_ties_to_int128(tie):
    w, K, kd, _ = B_TIES[tie]
    series = _b_series(tie)
    _assert_valid(series)
    for i, (c, h, lo) in enumerate(series):
        pairs, top = _bracket(c, w, K * kd, kd)
        # operands past 64 bits only: a one-tick outlier in a flat window ties as well, trivially
        wide = [(a, b) for a, b in pairs if max(a, b) >= 2**64]
        ties = sum(a == b for a, b in wide)
        below = sum(a < b for a, b in wide)
        above = sum(a > b for a, b in wide)
        assert ties >= 30 and below >= 30, (tie, i, ties, below, above)
        if tie == "w6":
            assert above >= 30, (tie, i, ties, below, above)
        if tie == "w3970" and i == 0:
            assert top > 2.0**110, top
            assert max(max(p) for p in pairs) > 2**110


@pytest.mark.parametrize("name", list(B_GRIDS))
def test_b_oracle_trades_below_the_tie_only(name):
    grid, series, oracle = _b_case(name)
    tie, offs, sl, tp, _ = B_GRIDS[name]
    nlev = len(sl) * len(tp)
    for i, (orc, _) in enumerate(oracle):
        n = np.array([int(o["n_trades"]) for o in orc]).reshape(len(offs), nlev)
        assert n.max() <= CAP_B
        # strict test: k below the tie trades at every untouched repetition, the tie never does
        below, tied = n[offs.index(-1)], n[offs.index(0)]
        assert (below >= tied + REPS // 3).all(), (name, i, n)
        if tie == "w6":  # the near ties on the L > R side trade on K as well
            assert (tied >= 30).all(), (name, i, n)
        else:
            assert (n[offs.index(0):] == 0).all(), (name, i, n)


@pytest.mark.parametrize("name", [n for n in B_GRIDS if B_GRIDS[n][0] != "w3970"])
def test_b_oracles_agree(name):
    grid, series, oracle = _b_case(name)
    for i, ((orc, _), ohlc) in enumerate(zip(oracle, series)):
        _assert_np_equal("boll", grid, ohlc, orc, f"B {name} series {i}")


def test_b_oracles_agree_at_the_2_32_edge():
    """oracle_np sums every window anew (O(bars x window)): the first two repetitions of the
    w = 3970 series, the second one a near tie."""
    w, K, kd, _ = B_TIES["w3970"]
    grid = D.Grid.boll([w], [K * kd - 1, K * kd], [9999], [9999], k_den=kd)
    c, h, lo = (x[:2 * (w + 3) + 5] for x in _b_series("w3970")[1])
    orc, _ = oracle_row("boll", grid, (c, h, lo, c), grid.annualization)
    assert [int(o["n_trades"]) for o in orc] == [2, 0]
    _assert_np_equal("boll", grid, (c, h, lo), orc, "B w3970 prefix")


def _accepted(grid):
    """bt_engine_create validates before it opens the device: an accepted grid gives an engine,
    or, on a machine without a GPU, the device error; a refused one its own message."""
    try:
        D.Engine(grid).close()
    except D.BtError as e:
        if not re.search("device|HIP", str(e)):
            raise
    return True


def test_b_window_times_k_limit():
    spec = r"outside the exact int128 range \(window \* k >= 2\^32\)"
    assert 4369 * 983055 == 2**32 - 1
    assert _accepted(D.Grid.boll([4369], [983055], [50], [50], k_den=2))
    assert _accepted(D.Grid.boll([4369], [2], [50], [50], k_den=983055))
    assert _accepted(D.Grid.boll([4095], [2**20], [50], [50], k_den=2**20))
    for name in B_GRIDS:
        grid = _b_case(name)[0]
        assert _accepted(grid) and len(grid.axes[1]) in (3, 12)
    for w, kn, kd in ((4096, 2**20, 2), (4096, 2, 2**20), (4369, 983056, 2), (4370, 983055, 2),
                      (4097, 2**20, 2)):
        with pytest.raises(D.BtError, match=spec):
            D.Engine(D.Grid.boll([w], [kn], [50], [50], k_den=kd))


@pytest.mark.gpu
@pytest.mark.parametrize("parity", [True, False])
@pytest.mark.parametrize("name", list(B_GRIDS))
def test_b_z_ties_gpu(name, parity):
    grid, series, oracle = _b_case(name)
    _gpu_check("boll", grid, series, oracle, "parity" if parity else 1, CAP_B, f"B {name}")
    if not parity:
        _gpu_check("boll", grid, series, oracle, 2, CAP_B, f"B {name}")


# ----------------------------------------------------------------------------------------- C
@pytest.mark.parametrize("strategy", list(C_GRIDS))
def test_c_prefix_ends_near_2_53(strategy):
    grid, series, oracle = _c_case(strategy)
    _assert_valid(series)
    c = series[0][0].astype(np.int64)
    assert len(c) == MAXB and c.min() >= 2**31 - 2**21
    assert 2**53 - 2**44 < int(c.sum()) < 2**53
    assert grid.n_params <= 8
    assert min(int(o["n_trades"]) for o in oracle[0][0]) >= 1000


@pytest.mark.gpu
@pytest.mark.parametrize("segments", [1, 0])
@pytest.mark.parametrize("strategy", list(C_GRIDS))
def test_c_maximum_length_gpu(strategy, segments):
    """Release instantiation, unsplit and with automatic segmentation. Measured: the C oracle
    takes 0.07-0.1 s per parameter on the CPU (18 parameters, 1.5 s, shared with the shape test);
    on an MI355X the unsplit runs with their oracle rows took 1.8 s (SMA, with the process's
    first device start), 0.44 s (EMA+OLS) and 0.49 s (Bollinger), the automatic ones 0.06-0.12 s:
    3.0 s for the six cases."""
    grid, series, oracle = _c_case(strategy)
    _gpu_check(strategy, grid, series, oracle, segments, 0, f"C {strategy}")


@pytest.mark.gpu
def test_c_one_bar_more_is_refused():
    with D.Engine(D.Grid.sma([2], [5])) as e:
        with pytest.raises(D.BtError, match="bad bar count"):
            e.load_ohlc([np.full(MAXB + 1, 1000, np.int32)])


# ----------------------------------------------------------------------------------------- D
@pytest.mark.parametrize("name", list(D_LIMITS))
def test_d_longest_accepted_window(name):
    wmax, word, mk = D_LIMITS[name]
    assert _accepted(mk(wmax))
    for w in (wmax + 1, wmax + 64, 2 * wmax):
        with pytest.raises(D.BtError, match=f"{word} grid needs more LDS than a CU has"):
            D.Engine(mk(w))
    # the GPU grids below sit on these limits
    if name in D_GRIDS:
        g = D_GRIDS[name][1]()
        assert max(g.axes[0 if name == "boll" else 1]) == wmax and _accepted(g)


@pytest.mark.parametrize("name", list(D_GRIDS))
def test_d_long_window_lanes_trade(name):
    strategy, grid, series, oracle = _d_case(name)
    _assert_valid(series)
    wmax = D_LIMITS[name][0]
    assert all(len(s[0]) == 3 * wmax + 77 for s in series)
    for p in range(grid.n_params):
        n = [int(orc[p]["n_trades"]) for orc, _ in oracle]
        assert max(n) <= CAP_D
        if wmax in grid.param(p).values():
            assert max(n) >= 1, (name, grid.param(p), n)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(D_GRIDS))
def test_d_longest_windows_gpu(name):
    strategy, grid, series, oracle = _d_case(name)
    _gpu_check(strategy, grid, series, oracle, "parity", CAP_D, f"D {name}")
