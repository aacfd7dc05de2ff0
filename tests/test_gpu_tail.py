"""Tail risk on the GPU (bt_tail / bt_tail_of, k_tail.hip; docs/tail_spec.md), every record field
for field against the Python-int reference of tail_ref.py, which works from the curves of
random_cases.lane_refs with a plain sorted: the random cases (all-lanes and list mode, both ways of
counting, the whole window and a cut one, one unit per chunk, both row homes, the identities with
the run's summaries and the covariance), crafted rows through tail_of at the smallest shapes at
which the selection and the sums can go wrong, the LDS boundary read from the plan driver, the ends
of the range (2^22 bars of +-(2^31 - 1), limit family A), ragged rows and the refusals. There is no
tolerance anywhere: every output is an integer.
tests/test_tail_cpu.py holds the host restatement to the same reference and proves that the cases
reach the shapes the selection can get wrong."""
import re

import numpy as np
import pytest

import dbx_amd as D
import random_cases as RC
import tail_ref as R
from helpers import build_plan_driver, run_driver

pytestmark = pytest.mark.gpu

LEVELS = R.LEVELS
assert LEVELS == (1, 10_000, 50_000, 250_000, 500_000, 1_000_000, 50_000, 999_999)
Q = len(LEVELS)
BIG = 2**31 - 1


def _load(e, strategy, series, ids=None):
    """series: [(h, l, c)]."""
    closes = [s[2] for s in series]
    if strategy == "boll":
        e.load_ohlc(closes, [s[0] for s in series], [s[1] for s in series], sym_ids=ids)
    else:
        e.load_ohlc(closes, sym_ids=ids)


def _plan(*args):
    """units P Q list staged longest_n cus row_req budget_req -> the TailPlan."""
    return run_driver(build_plan_driver("tail_plan_driver"), *args)


def _same(got, recs, qs, where):
    R.assert_same(got.lanes, recs, f"{where}: records")
    R.assert_same(got.quantiles, qs, f"{where}: quantiles")
    assert got.levels_ppm.tolist() == list(LEVELS)


def _bytes(tr):
    return tr.lanes.tobytes(), tr.quantiles.tobytes()


def _settings(e, call, want, where, budget, pitch_budget):
    """The same bytes with one unit per chunk and under both row homes. `budget`: one unit with the
    row in LDS; `pitch_budget`: one unit with the row in the arena."""
    for row, bud in ((0, budget), (1, 0), (2, 0), (2, pitch_budget)):
        e.set_tail_row(row)
        e.set_tail_budget(bud)
        try:
            got = call()
            assert e.last_tail_row() == (2 if row == 2 else 1), f"{where}: row home under set_tail_row({row})"
        finally:
            e.set_tail_row(0)
            e.set_tail_budget(0)
        assert _bytes(got) == want, f"{where}: set_tail_row({row}), budget {bud}"


# ------------------------------------------------------------------------ 1. the random cases
@pytest.mark.parametrize("strategy,seed", RC.CASES)
def test_random_cases(strategy, seed):
    c = RC.lane_case(strategy, seed)
    where = f"{strategy} seed {seed}"
    S, P = len(c.series), c.grid.n_params
    with D.Engine(c.grid, topk=c.topk) as e:
        _load(e, strategy, c.series, c.ids)
        e.run()
        before = (e.summaries().tobytes(), e.read_topk().tobytes())
        out = {}
        for held in (False, True):
            for cut in (False, True):
                recs, qs, window = R.random_refs(strategy, seed, held, cut)
                w = f"{where}, held={held}, window={window}"
                got = e.tail_risk(LEVELS, window=window, held=held)
                _same(got, recs, qs, f"{w}: all-lanes")
                lrecs, lqs = R.list_refs(c, recs, qs)
                lst = e.tail_risk(LEVELS, c.replay_lanes, window=window, held=held)
                _same(lst, lrecs, lqs, f"{w}: list mode")
                longest = max(min(window[1], max(c.bars)) - window[0], 0) if window else max(c.bars)
                pitch = -(-longest // 64) * 64
                _settings(e, lambda: e.tail_risk(LEVELS, window=window, held=held), _bytes(got), f"{w}: all-lanes",
                          R.rows_budget(P, Q, 0, 1), R.rows_budget(P, Q, pitch, 1))
                _settings(e, lambda: e.tail_risk(LEVELS, c.replay_lanes, window=window, held=held), _bytes(lst),
                          f"{w}: list mode", R.rows_budget(1, Q, 0, 1, True), R.rows_budget(1, Q, pitch, 1, True))
                out[held, cut] = got
        # the identities with what the sweep kernels and the covariance produce
        every, heldr = out[False, False], out[True, False]
        assert np.array_equal(every.lanes["s1"], e.summaries()["pnl"]), f"{where}: s1 against summaries()"
        assert np.array_equal(every.lanes["n"], np.repeat(np.array(c.bars)[:, None], P, 1)), where
        cov = e.covariance(c.cov_lanes)
        row = {i: s for s, i in enumerate(c.ids)}
        assert [every.s2[row[i], p] for i, p in c.cov_lanes] == np.diag(cov.gram).tolist(), f"{where}: s2 against covariance()"
        for f in D.TAIL_DTYPE.names:    # held mode drops only zeros
            if f not in ("n", "n_window", "min_bar", "max_bar", "min_d", "max_d"):
                assert np.array_equal(every.lanes[f], heldr.lanes[f]), f"{where}: {f} differs between the two modes"
        a1, a6 = every.quantiles[..., 0], every.quantiles[..., 5]      # 1 ppm and 10^6 ppm
        assert np.array_equal(a1["var"], every.lanes["min_d"]) and np.array_equal(a6["var"], every.lanes["max_d"]), where
        assert np.array_equal(a6["es_sum"], every.lanes["s1"]), where
        assert (e.summaries().tobytes(), e.read_topk().tobytes()) == before, f"{where}: the run's results changed"


# ------------------------------------------------------------ 2. crafted rows through tail_of
def _crafted():
    """{name: rows of one length}: each the smallest shape at which one step can go wrong."""
    rows = {}
    for T_ in (1, 2, 63, 64, 65, 128, 129):
        rng = np.random.default_rng([0x7A11, T_])
        rows[f"T{T_}"] = [rng.integers(-1000, 1000, T_), np.full(T_, -7), np.zeros(T_, np.int64), np.full(T_, 12345),
                          np.where(np.arange(T_) % 2 == 0, BIG, -BIG)]
    base = np.arange(200) % 2
    rows["two_values"] = [np.where(base == 1, 0x01020304, 0x01020305),          # the lowest byte
                          np.where(base == 1, 0x01020304, 0x7F020304),          # the top byte
                          np.where(base == 1, -0x01020304, -0x7F020304),
                          np.where(base == 1, -1, 0),                           # the sign
                          np.where(np.arange(200) % 3 == 0, -1, 0)]
    rows["monotone"] = [np.arange(300) * 7 - 1000, 1000 - np.arange(300) * 7]
    # ties: 100 bars with -5 at indices 10..29 sorted first; k = 1 (first of the run) at 1 % and
    # k = 20 (its last element) at 20 %, k = 21 the first of the next run
    tie = np.full(100, 3)
    tie[10:30] = -5
    tie[40:60] = 9
    rows["ties"] = [tie, -tie]
    return {k: np.array(v, np.int64) for k, v in rows.items()}


TIE_LEVELS = (10_000, 200_000, 210_000, 800_000, 810_000, 1_000_000)


@pytest.mark.parametrize("row", (1, 2))
def test_crafted_rows_through_tail_of(row):
    with D.Engine(D.Grid.sma([2], [5])) as e:
        e.set_tail_row(row)
        for name, d in _crafted().items():
            for levels in (LEVELS, TIE_LEVELS, (50_000,), (50_000,) * 8):
                recs, qs = R.rows_tail(d, levels)
                got = e.tail_of(d, levels)
                assert e.last_tail_row() == row
                R.assert_same(got.lanes, recs, f"{name}, row home {row}, levels {levels}: records")
                R.assert_same(got.quantiles, qs, f"{name}, row home {row}, levels {levels}: quantiles")
            if name == "T1":
                assert (got.quantiles["k"] == 1).all()
                assert np.array_equal(got.quantiles["var"][:, 0], d[:, 0]) and np.array_equal(got.quantiles["es_sum"][:, 0], d[:, 0])
        recs, qs = R.rows_tail(_crafted()["ties"], TIE_LEVELS)
        assert qs["k"][0].tolist() == [1, 20, 21, 80, 81, 100] and qs["n_lt"][0].tolist() == [0, 0, 20, 20, 80, 80]


# ------------------------------------------------------------------------- 3. the LDS boundary
def test_rows_at_the_lds_capacity_and_one_above():
    cap = _plan(1, 1, 2, 0, 1, 100, 256, 0, 0)["lds_row_cap"]
    assert _plan(1, 1, 2, 0, 1, cap, 256, 0, 0)["row_mode"] == 1 and _plan(1, 1, 2, 0, 1, cap + 1, 256, 0, 0)["row_mode"] == 2
    rng = np.random.default_rng(0x7A12)
    with D.Engine(D.Grid.sma([2], [5])) as e:
        assert e.last_tail_row() == 0
        for T_, home in ((cap, 1), (cap + 1, 2)):
            d = rng.integers(-50_000, 50_000, (2, T_))
            recs, qs = R.rows_tail(d, (1, 50_000, 1_000_000))
            got = e.tail_of(d, (1, 50_000, 1_000_000))
            assert e.last_tail_row() == home, f"T = {T_}"
            R.assert_same(got.lanes, recs, f"T = {T_}: records")
            R.assert_same(got.quantiles, qs, f"T = {T_}: quantiles")
        e.set_tail_row(1)
        with pytest.raises(D.BtError, match=rf"a row of {cap + 1} counted bars \({4 * (cap + 1)} bytes\) does not fit the {4 * cap} bytes"):
            e.tail_of(d, (50_000,))
        e.set_tail_row(0)
        assert e.tail_of(d, (1, 50_000, 1_000_000)).quantiles.tobytes() == got.quantiles.tobytes()


# ---------------------------------------------------------------------- 4. the ends of the range
@pytest.mark.parametrize("T_", (70_000, 1 << 22))
def test_the_largest_increments_on_the_longest_row(T_):
    """d = +-(2^31 - 1) alternating: s4 fills the third word, s3 cancels to its exact value, es_sum
    sits near -2^52 at 2^22 bars. The reference is closed form (a Python sum of 4M fourth powers
    would take longer than the test may)."""
    d = np.where(np.arange(T_ + 1) % 2 == 0, -BIG, BIG).astype(np.int64)[None, :T_]
    d = np.concatenate([d, -d])                    # the second row starts with +BIG
    levels = (1, 500_000, 500_001, 1_000_000)
    with D.Engine(D.Grid.sma([2], [5])) as e:
        got = e.tail_of(d, levels)
        assert e.last_tail_row() == 2
    h = T_ // 2
    ks = [-(-T_ * a // 1_000_000) for a in levels]
    assert ks[1] == h and ks[0] < h < ks[2] and ks[3] == T_
    for i in range(2):
        r, q = got.lanes[i], got.quantiles[i]
        assert (int(r["n"]), int(r["n_window"]), int(r["n_pos"]), int(r["n_neg"])) == (T_, T_, h, h)
        assert (int(r["min_d"]), int(r["max_d"]), int(r["min_bar"]), int(r["max_bar"])) == (-BIG, BIG, i, 1 - i)
        assert (int(r["s1"]), int(r["s1_neg"]), R.wide(r, "s3")) == (0, -h * BIG, 0)
        assert (R.wide(r, "s2"), R.wide(r, "s2_neg"), R.s4_of(r)) == (T_ * BIG**2, h * BIG**2, T_ * BIG**4)
        assert q["k"].tolist() == ks and q["n_lt"].tolist() == [0 if k <= h else h for k in ks]
        assert q["var"].tolist() == [-BIG if k <= h else BIG for k in ks]
        assert q["es_sum"].tolist() == [(max(k - h, 0) - min(k, h)) * BIG for k in ks]
    if T_ == 1 << 22:
        assert int(got.lanes[0]["s4"][2]) > 0 and -2**52 <= int(got.quantiles[0, 1]["es_sum"]) < -2**51
    # an odd row: s3 does not cancel
    with D.Engine(D.Grid.sma([2], [5])) as e:
        odd = e.tail_of(d[:, :T_ - 1], levels).lanes
    assert [R.wide(r, "s3") for r in odd] == [-BIG**3, BIG**3] and [int(r["s1"]) for r in odd] == [-BIG, BIG]


@pytest.mark.parametrize("name", ("sma", "ema_ols", "boll"))
def test_family_a_touches_the_top_key_byte_on_real_walks(name):
    grid, series, curves = R.family_a_curves(name)
    S, P = len(series), grid.n_params
    assert max(abs(int(x)) for _, eq in curves for x in np.diff(eq, prepend=0)) >= 2**30 or name == "ema_ols"
    with D.Engine(grid) as e:
        _load(e, name, [(h, lo, c) for c, h, lo in series])
        for held in (False, True):
            recs, qs = R.lanes_tail(curves, None, held)
            got = e.tail_risk(LEVELS, held=held)
            _same(got, recs.reshape(S, P), qs.reshape(S, P, Q), f"family A {name}, held={held}")
            e.set_tail_row(2)
            assert _bytes(e.tail_risk(LEVELS, held=held)) == _bytes(got)
            e.set_tail_row(0)


# ------------------------------------------------------------------------------ 5. ragged rows
@pytest.mark.parametrize("strategy", RC.STRATEGIES)
def test_ragged_rows_and_empty_windows(strategy):
    grid, series, curves = R.ragged_curves(strategy)
    S, P = len(series), grid.n_params
    zero, zq = np.zeros((), D.TAIL_DTYPE), np.zeros(Q, D.TAIL_Q_DTYPE)
    zero["min_bar"] = zero["max_bar"] = -1
    with D.Engine(grid) as e:
        _load(e, strategy, series)
        for window in (None, (1, 64), (64, 66), (65, 1000), (700, 701), (5000, 6000)):
            for held in (False, True):
                recs, qs = R.lanes_tail(curves, window, held)
                for row in (1, 2):
                    e.set_tail_row(row)
                    got = e.tail_risk(LEVELS, window=window, held=held)
                    _same(got, recs.reshape(S, P), qs.reshape(S, P, Q), f"{strategy}, window {window}, held={held}, row {row}")
                e.set_tail_row(0)
                lanes = got.lanes.reshape(-1)
                empty = lanes["n"] == 0
                assert all(x.tobytes() == zero.tobytes() for x in lanes[empty & (lanes["n_window"] == 0)])
                assert all(x.tobytes() == zq.tobytes() for x in got.quantiles.reshape(-1, Q)[empty])
                if window == (5000, 6000):
                    assert empty.all() and not lanes["n_window"].any()
                if window is None and not held:      # the 1-bar row: one counted bar with d = 0
                    assert (got.lanes[0]["n"] == 1).all() and (got.quantiles[0]["k"] == 1).all()
                if window is None and held:          # lanes that never trade count no bar
                    never = recs["n_pos"] + recs["n_neg"] == 0
                    assert never.sum() >= 1 and (got.lanes[0]["n"] == 0).all()


# ------------------------------------------------------------------------------- 6. refusals
def test_refusals_name_the_value_and_leave_the_engine_usable():
    c = RC.lane_case("sma", 0)
    recs, qs, _ = R.random_refs("sma", 0)
    with D.Engine(c.grid) as e:
        with pytest.raises(D.BtError, match="bt_tail: no dataset loaded"):
            e.tail_risk(LEVELS)
        assert e.tail_of([[1, -2, 3]], (500_000,)).quantiles["var"].tolist() == [[1]]   # needs no dataset
        _load(e, "sma", c.series, c.ids)
        lane = [(c.ids[0], 0)]
        for kw, named in (
            (dict(levels=()), r"Q = 0 outside \[1, 8\]"),
            (dict(levels=(1,) * 9), r"Q = 9 outside \[1, 8\]"),
            (dict(levels=(5, 0)), r"level 1: alpha_ppm = 0 outside \[1, 1000000\]"),
            (dict(levels=(1_000_001,)), r"level 0: alpha_ppm = 1000001 outside"),
            (dict(levels=(0.5, 2.0)), r"level 1: alpha_ppm = 2000000 outside"),
            (dict(window=(-1, 5)), r"window \[-1, 5\) is empty or negative"),
            (dict(window=(7, 7)), r"window \[7, 7\) is empty or negative"),
            (dict(window=(9, 3)), r"window \[9, 3\) is empty or negative"),
            (dict(lanes=[]), r"n = 0 outside \[1, 1048576\]"),
            (dict(lanes=[(10**6, 0)]), r"unknown symbol id 1000000 \(lane 0\)"),
            (dict(lanes=[(c.ids[0], c.grid.n_params)]), rf"param {c.grid.n_params} outside \[0, {c.grid.n_params}\)"),
        ):
            with pytest.raises(D.BtError, match=named):
                e.tail_risk(**{"levels": LEVELS, **kw})
            assert e.tail_risk(LEVELS, lane).lanes.tobytes() == recs[0, :1].tobytes()
        f = D.engine.sym("bt_tail")
        lv = np.array(LEVELS, np.int32)
        out = np.zeros(len(c.series) * c.grid.n_params, D.TAIL_DTYPE)
        for args, named in (((0, None, 0, 0, 2, Q, lv.ctypes.data, out.ctypes.data, None), "mode = 2 is neither"),
                            ((0, None, 0, 0, 0, Q, None, out.ctypes.data, None), "alpha_ppm is NULL"),
                            ((3, None, 0, 0, 0, Q, lv.ctypes.data, out.ctypes.data, None), r"n = 3 with lanes == NULL"),
                            ((0, None, 0, 0, 0, Q, lv.ctypes.data, None, None), "recs_out and q_out are both NULL")):
            assert f(e._h, *args) == -1
            assert re.search(named, D.lib().bt_last_error().decode()), D.lib().bt_last_error().decode()
        assert f(e._h, 0, None, 0, 0, 0, Q, lv.ctypes.data, out.ctypes.data, None) == 0      # the records alone
        assert out.tobytes() == recs.tobytes()
        with pytest.raises(D.BtError, match=r"d\[1\]\[2\] = -2147483648 outside the domain"):
            e.tail_of([[0, 1, 2], [3, 4, -2**31]], (5,))
        for d, named in ((np.zeros((0, 4), np.int64), r"n = 0 outside"), (np.zeros((2, 0), np.int64), r"T = 0 outside")):
            with pytest.raises(D.BtError, match=named):
                e.tail_of(d, (5,))
        with pytest.raises(D.BtError, match=r"mode = 3 outside \[0, 2\]"):
            e.set_tail_row(3)
        with pytest.raises(D.BtError, match="bytes = -1 is negative"):
            e.set_tail_budget(-1)
        e.set_tail_budget(2000)
        with pytest.raises(D.BtError, match=r"the staging of one dataset row \(\d+ bytes\) exceeds the budget of 2000 bytes"):
            e.tail_risk(LEVELS)
        e.set_tail_budget(0)
        _same(e.tail_risk(LEVELS), recs, qs, "after the refusals")
