"""The drawdown bootstrap on the GPU (bt_drawdown_boot / bt_drawdown_boot_of, k_ddboot.hip;
docs/drawdown_spec.md), byte for byte against the Python-int reference of ddboot_ref.py, which draws
the bars one by one and walks every resampled path: staged rows at the smallest shapes at which the
tables, the resampling, the reduction and the selection can go wrong, crafted rows with closed
forms and their tie to the reality check, the ends of the range, B = 65,536, the LDS boundary read
from the plan driver, and the walked path on the random cases, ragged rows and window edges, in both
row homes and with one lane per chunk. There is no tolerance anywhere: every output is an integer.
tests/test_ddboot_cpu.py holds the host restatement to the same reference and proves that the cases
reach the shapes the kernel can get wrong."""
import re

import numpy as np
import pytest

import dbx_amd as D
import bootstrap_ref as BR
import ddboot_ref as R
import random_cases as RC
from helpers import build_plan_driver, run_driver

pytestmark = pytest.mark.gpu

LEVELS, LIMITS = R.LEVELS, R.LIMITS
Q, NR = len(LEVELS), len(LIMITS)
BIG = R.BIG


def _load(e, strategy, series, ids=None):
    """series: [(h, l, c)]."""
    closes = [s[2] for s in series]
    if strategy == "boll":
        e.load_ohlc(closes, [s[0] for s in series], [s[1] for s in series], sym_ids=ids)
    else:
        e.load_ohlc(closes, sym_ids=ids)


def _plan(n, T, B, L, Q_=Q, R_=NR, lst=0, staged=0, raw=0, row=0, budget=0):
    return run_driver(build_plan_driver("ddboot_plan_driver"), n, T, B, L, Q_, R_, lst, staged, raw, 256, row, budget)


def _one_lane(n, T, B, L, row, **kw):
    """The budget under which a call of n lanes runs one lane per chunk with the row home `row`."""
    pl = _plan(n, T, B, L, row=row, **kw)
    budget = pl["need_bytes"] + pl["unit_bytes"] - 1
    assert _plan(n, T, B, L, row=row, budget=budget, **kw)["chunks"] == n
    return budget


def _settings(e, call, want, where, n, T, B, L, chunks=(False, True), **kw):
    """The same bytes in both row homes and with one lane per chunk."""
    for row in (0, 1, 2):
        for chunked in chunks:
            e.set_ddboot_row(row)
            e.set_ddboot_budget(_one_lane(n, T, B, L, row, **kw) if chunked else 0)
            try:
                got = call()
                home = e.last_ddboot_row()
            finally:
                e.set_ddboot_row(0)
                e.set_ddboot_budget(0)
            assert home == _plan(n, T, B, L, row=row, **kw)["row_mode"] and (row == 0 or home == row), where
            assert R.out_bytes(got) == want, f"{where}: set_ddboot_row({row}), one lane per chunk: {chunked}"


@pytest.fixture(scope="module")
def eng():
    with D.Engine(D.Grid.sma([2], [5])) as e:
        yield e


# --------------------------------------------------------------------------- 1. staged shapes
@pytest.mark.parametrize("T", R.OF_T)
def test_staged_shapes(eng, T):
    cases = R.of_cases(T)
    assert {c[0] for c in cases} == set(R.of_L(T)) and {c[1] for c in cases} == set(R.OF_B) and {c[2] for c in cases} == {1, 3}
    for k, (L, B, n, seed) in enumerate(cases):
        where = f"T = {T}, L = {L}, B = {B}, n = {n}"
        d, want = R.of_rows(T, n), R.of_ref(T, k)
        call = lambda raw=True: eng.drawdown_of(d, B, L, seed, LEVELS, LIMITS, raw=raw)
        got = call()
        R.assert_same(got, want, where)
        assert got.levels_ppm.tolist() == list(LEVELS) and got.limits.tolist() == list(LIMITS) and got.resamples == B
        _settings(eng, call, R.out_bytes(got), where, n, T, B, L, staged=1, raw=1)
        # without raw the values of the selection live elsewhere: the same figures
        lean = call(False)
        assert lean.raw is None and R.out_bytes(lean)[:3] == R.out_bytes(got)[:3], where
        _settings(eng, lambda: call(False), R.out_bytes(lean), f"{where}, no raw", n, T, B, L, chunks=(n > 1,), staged=1)
        # each output alone
        alone = eng.drawdown_of(d, B, L, seed, (), (), raw=False)
        assert alone.lanes.tobytes() == got.lanes.tobytes() and alone.quantiles.size == 0 == alone.reach.size, where


# ----------------------------------------------------------------------------- 2. crafted rows
def test_crafted_rows(eng):
    for name, (rows, B, L, seed) in R.crafted().items():
        n, T = rows.shape
        want = R.drawdown_risk(rows.tolist(), B, L, seed)
        call = lambda: eng.drawdown_of(rows, B, L, seed, LEVELS, LIMITS, raw=True)
        got = call()
        R.assert_same(got, want, name)
        _settings(eng, call, R.out_bytes(got), name, n, T, B, L, staged=1, raw=1)
        boot = eng.bootstrap_of(rows, None, B, L, seed, boot=True).boot      # the same bars
        assert (got.raw >= np.maximum(0, -boot)).all(), f"{name}: MDD* is at least the loss of the whole path"
        if name == "nonneg":
            assert not got.raw.any() and not got.lanes["mdd"].any() and (got.lanes["n_ge"] == B).all()
        if name == "constant_neg":
            assert (got.raw == -rows[:, :1] * T).all() and (got.lanes["min_star"] == got.lanes["max_star"]).all()
            assert got.m1.tolist() == [B * -int(c) * T for c in rows[:, 0]]
        if name in ("constant_neg", "nonpos"):
            assert np.array_equal(got.raw, -boot), f"{name}: a path that never rises draws down by its sum"
        if name.startswith("rotation"):
            assert _plan(n, T, B, L, staged=1)["K"] == 1


# ------------------------------------------------------------------------ 3. the ends of the range
def test_the_largest_increments(eng):
    T, B, L = 4096, 64, 33
    alt = np.where(np.arange(T) % 2 == 0, -BIG, BIG)
    for name, rows in (("constant", np.stack([np.full(T, BIG), np.full(T, -BIG)])), ("alternating", np.stack([alt, -alt]))):
        want = R.drawdown_risk(rows.tolist(), B, L, 0xB16)
        call = lambda: eng.drawdown_of(rows, B, L, 0xB16, LEVELS, LIMITS, raw=True)
        got = call()
        R.assert_same(got, want, name)
        assert eng.last_ddboot_row() == 2
        eng.set_ddboot_row(1)           # 229 KB of row and tables: more than a CU's LDS
        try:
            with pytest.raises(D.BtError, match=r"T = 4096 bars \(229384 bytes\) do not fit the LDS row limit"):
                call()
        finally:
            eng.set_ddboot_row(0)
        assert R.out_bytes(call()) == R.out_bytes(got), f"{name}: after the refusal"
        if name == "constant":
            assert got.raw[0].tolist() == [0] * B and got.raw[1].tolist() == [BIG * T] * B


def test_the_longest_row_in_closed_form(eng):
    """2^22 bars of -(2^31 - 1): every path falls by (2^31 - 1) 2^22 whatever it draws; of +(2^31 - 1):
    no path ever falls."""
    T, B, L = 1 << 22, 64, 4096
    rows = np.stack([np.full(T, -BIG, np.int32), np.full(T, BIG, np.int32)])
    got = eng.drawdown_of(rows, B, L, 7, (500_000, 1_000_000), (BIG * T, BIG * T + 1))
    assert eng.last_ddboot_row() == 2
    down, up = got.lanes
    deep = BIG * T
    assert (int(down["sum"]), int(down["mdd"]), int(down["n_ge"]), int(down["min_star"]), int(down["max_star"])) == \
        (-deep, deep, B, deep, deep)
    assert got.m1.tolist() == [B * BIG * 2**22, 0] and got.m2.tolist() == [B * deep * deep, 0]
    assert (int(up["sum"]), int(up["mdd"]), int(up["n_ge"]), int(up["min_star"]), int(up["max_star"])) == (deep, 0, B, 0, 0)
    assert got.quantiles.tolist() == [[deep, deep], [0, 0]] and got.reach.tolist() == [[B, 0], [0, 0]]


# ------------------------------------------------------------------------- 4. the most resamples
def test_the_most_resamples(eng):
    T, B, L = 8, 65_536, 3
    rows = np.array([[3, -5, 2, -4, 6, 1, -7, 2], [-1, 0, 0, 2, -2, 0, 1, -1]])
    levels = (1, 250_000, 500_000, 500_001, 999_999, 1_000_000)
    want = R.drawdown_risk(rows.tolist(), B, L, 0x10000, levels, (0, 7, 12, 40))
    got = eng.drawdown_of(rows, B, L, 0x10000, levels, (0, 7, 12, 40), raw=True)
    R.assert_same(got, want, "B = 65536")
    lean = eng.drawdown_of(rows, B, L, 0x10000, levels, (0, 7, 12, 40))
    assert R.out_bytes(lean)[:3] == R.out_bytes(got)[:3]
    with pytest.raises(D.BtError, match=r"B = 65537 outside \[1, 65536\]"):
        eng.drawdown_of(rows, B + 1, L)


def test_values_above_64_kb_of_lds_in_both_homes(eng):
    """B = 8,192 without raw: the values of the selection take 64 KB of LDS behind the scratch, so the
    workgroup passes the 64 KB a kernel gets unasked whether the row is in LDS or in the arena."""
    T, B, L = 8, 8192, 3
    rows = np.array([[3, -5, 2, -4, 6, 1, -7, 2], [-1, 0, 0, 2, -2, 0, 1, -1], [0, 9, -9, 9, -9, 0, 0, -1]])
    want = R.drawdown_risk(rows.tolist(), B, L, 0x2000)
    for row, home in ((0, 1), (1, 1), (2, 2)):
        pl = _plan(3, T, B, L, staged=1, row=row)
        assert pl["row_mode"] == home and pl["l_vals"] > 0 and pl["v_pitch"] == 0 and 64 * 1024 < pl["lds_bytes"] <= 160 * 1024
        eng.set_ddboot_row(row)
        try:
            got = eng.drawdown_of(rows, B, L, 0x2000, LEVELS, LIMITS)
            assert eng.last_ddboot_row() == home
        finally:
            eng.set_ddboot_row(0)
        R.assert_same(got, want, f"B = 8192, set_ddboot_row({row})", raw=False)
    # a walked lane the same way
    c = RC.lane_case("sma", 0)
    d, _ = R.lane_increments("sma", 0, (0, 64))
    lane_ref = R.drawdown_risk(d[:2], B, 10, 5)
    with D.Engine(c.grid) as e:
        _load(e, "sma", c.series, c.ids)
        for row in (1, 2):
            e.set_ddboot_row(row)
            got = e.drawdown_risk([(c.ids[0], 0), (c.ids[0], 1)], B, 10, 5, (0, 64), LEVELS, LIMITS)
            assert e.last_ddboot_row() == row
            R.assert_same(got, lane_ref, f"walked lanes, B = 8192, set_ddboot_row({row})", raw=False)


# ---------------------------------------------------------------------------- 5. the LDS boundary
def test_rows_at_the_lds_capacity_and_one_above(eng):
    pl = _plan(2, 100, 16, 1, staged=1)
    assert pl["two_tables"] == 0 and pl["entry_bytes"] == 24
    cap = (pl["lds_cap_bytes"] - pl["fixed_bytes"] - 8) // (8 + pl["entry_bytes"])
    assert _plan(2, cap, 16, 1, staged=1)["row_mode"] == 1 and _plan(2, cap + 1, 16, 1, staged=1)["row_mode"] == 2
    rng = np.random.default_rng(0xDD12)
    for T, home in ((cap, 1), (cap + 1, 2)):
        d = rng.integers(-50_000, 50_000, (2, T))
        want = R.drawdown_risk(d.tolist(), 16, 1, 3)
        got = eng.drawdown_of(d, 16, 1, 3, LEVELS, LIMITS, raw=True)
        assert eng.last_ddboot_row() == home, f"T = {T}"
        R.assert_same(got, want, f"T = {T}")
    # forced into LDS: refused one bar above the capacity
    eng.set_ddboot_row(1)
    try:
        with pytest.raises(D.BtError, match=rf"the prefix row and block tables of T = {cap + 1} bars \(\d+ bytes\) do not fit the LDS row limit"):
            eng.drawdown_of(d, 16, 1, 3)
    finally:
        eng.set_ddboot_row(0)
    assert R.out_bytes(eng.drawdown_of(d, 16, 1, 3, LEVELS, LIMITS, raw=True)) == R.out_bytes(got)


# ------------------------------------------------------------------------------- 6. walked lanes
@pytest.mark.parametrize("strategy,seed", RC.CASES)
def test_random_cases(strategy, seed):
    c = RC.lane_case(strategy, seed)
    where = f"{strategy} seed {seed}"
    S, P = len(c.series), c.grid.n_params
    B, L, sd = R.walk_params(strategy, seed)
    with D.Engine(c.grid, topk=c.topk) as e:
        _load(e, strategy, c.series, c.ids)
        e.run()
        before = (e.summaries().tobytes(), e.read_topk().tobytes())
        for cut in (False, True):
            want, window = R.walk_ref(strategy, seed, cut)
            T = window[1] - window[0] if window else max(c.bars)
            w = f"{where}, window {window}"
            got = e.drawdown_risk(None, B, L, sd, window, LEVELS, LIMITS)
            assert got.lanes.shape == (S, P) and got.quantiles.shape == (S, P, Q) and got.raw is None
            R.assert_same(got, want, f"{w}: all-lanes", raw=False)
            flat = [row * P + p for row, p in ((c.ids.index(i), p) for i, p in c.replay_lanes)]
            lst = e.drawdown_risk(c.replay_lanes, B, L, sd, window or (0, max(c.bars)), LEVELS, LIMITS, raw=True)
            for name in ("lanes", "quantiles", "reach", "raw"):
                assert getattr(lst, name).tobytes() == getattr(want, name)[flat].tobytes(), f"{w}: list mode, {name}"
            if seed < 2:
                _settings(e, lambda: e.drawdown_risk(None, B, L, sd, window, LEVELS, LIMITS), R.out_bytes(got), f"{w}: all-lanes",
                          S * P, T, B, L)
        every, _ = R.walk_ref(strategy, seed)
        got = e.drawdown_risk(None, B, L, sd, None, LEVELS, LIMITS)
        assert np.array_equal(got.lanes["mdd"], e.summaries()["mdd"]), f"{where}: mdd against summaries()"
        assert np.array_equal(got.lanes["sum"], e.summaries()["pnl"]), f"{where}: sum against summaries()"
        assert (e.summaries().tobytes(), e.read_topk().tobytes()) == before, f"{where}: the run's results changed"
    # two engines holding half the rows each, one explicit window: the shards concatenate
    window = (0, max(c.bars))
    parts = []
    for rows in (range(0, S // 2), range(S // 2, S)):
        with D.Engine(c.grid) as e:
            _load(e, strategy, [c.series[s] for s in rows], [c.ids[s] for s in rows])
            parts.append(e.drawdown_risk(None, B, L, sd, window, LEVELS, LIMITS))
    for name in ("lanes", "quantiles", "reach"):
        both = np.concatenate([getattr(p, name) for p in parts])
        assert both.tobytes() == getattr(every, name).reshape(both.shape).tobytes(), f"{where}: two shards, {name}"


@pytest.mark.parametrize("strategy", RC.STRATEGIES)
def test_window_edges_on_ragged_rows(strategy):
    c = BR.edge_case(strategy)
    P = c.grid.n_params
    with D.Engine(c.grid) as e:
        _load(e, strategy, c.series)
        for frm, to in R.EDGE_WINDOWS:
            want = R.edge_ref(strategy, frm, to)
            sd = R.EDGE.seed + 1000 * frm + to
            for row in (1, 2):
                e.set_ddboot_row(row)
                got = e.drawdown_risk(None, R.EDGE.B, R.EDGE.L, sd, (frm, to), LEVELS, LIMITS)
                R.assert_same(got, want, f"{strategy}, window [{frm}, {to}), row home {row}", raw=False)
            e.set_ddboot_row(0)
            ended = np.repeat(np.array(c.bars) <= frm, P)             # rows that end before the window: no bar moves
            assert not got.lanes.reshape(-1)[ended]["max_star"].any() and ended.any() == (frm >= 1)


# --------------------------------------------------------------------------------- 7. refusals
def test_refusals_name_the_value_and_leave_the_engine_usable():
    c = RC.lane_case("sma", 0)
    B, L, sd = R.walk_params("sma", 0)
    want, _ = R.walk_ref("sma", 0)
    with D.Engine(c.grid) as e:
        with pytest.raises(D.BtError, match="bt_drawdown_boot: no dataset loaded"):
            e.drawdown_risk()
        small = R.drawdown_risk([[1, -2, 3]], 5, 2, 0, (1_000_000,), ())
        assert e.drawdown_of([[1, -2, 3]], 5, 2, levels=(1.0,)).quantiles.tolist() == small.quantiles.tolist()   # needs no dataset
        _load(e, "sma", c.series, c.ids)
        lane = [(c.ids[0], 0)]
        for kw, named in (
            (dict(levels=(1,) * 9), r"Q = 9 outside \[0, 8\]"),
            (dict(limits=(1,) * 9), r"R = 9 outside \[0, 8\]"),
            (dict(levels=(5, 0)), r"level 1: alpha_ppm = 0 outside \[1, 1000000\]"),
            (dict(levels=(0.5, 2.0)), r"level 1: alpha_ppm = 2000000 outside"),
            (dict(limits=(3, 0, -1)), r"limit 2: -1 is negative"),
            (dict(resamples=0), r"B = 0 outside \[1, 65536\]"),
            (dict(block=0), r"L = 0 outside \[1, 4194304\]"),
            (dict(block=(1 << 22) + 1), r"L = 4194305 outside"),
            (dict(window=(-1, 5)), r"from_bar = -1 is negative"),
            (dict(window=(7, 7)), r"T = 0 bars of the window \[7, 7\) outside \[1, 4194304\]"),
            (dict(window=(0, (1 << 22) + 1)), r"T = 4194305 bars"),
            (dict(lanes=[]), r"n = 0 outside \[1, 1048576\]"),
            (dict(lanes=[(10**6, 0)]), r"unknown symbol id 1000000 \(lane 0\)"),
            (dict(lanes=[(c.ids[0], c.grid.n_params)]), rf"param {c.grid.n_params} outside \[0, {c.grid.n_params}\)"),
        ):
            with pytest.raises(D.BtError, match=named):
                e.drawdown_risk(**{"resamples": B, "block": L, "seed": sd, **kw})
            got = e.drawdown_risk(lane, B, L, sd, (0, max(c.bars)), LEVELS, LIMITS)
            assert got.lanes.tobytes() == want.lanes[:1].tobytes(), named
        with pytest.raises(ValueError, match="raw comes with lanes only"):
            e.drawdown_risk(raw=True)
        f = D.engine.sym("bt_drawdown_boot")
        lv, lm = np.array(LEVELS, np.int32), np.array(LIMITS, np.int64)
        n = len(c.series) * c.grid.n_params
        out, raw = np.zeros(n, D.DD_LANE_DTYPE), np.zeros(n * B, np.int64)
        for args, named in (((0, None, 0, 0, B, L, sd, Q, None, 0, None, out.ctypes.data, None, None, None), "alpha_ppm is NULL"),
                            ((0, None, 0, 0, B, L, sd, 0, None, 1, None, out.ctypes.data, None, None, None), "limits is NULL"),
                            ((3, None, 0, 0, B, L, sd, 0, None, 0, None, out.ctypes.data, None, None, None), r"n = 3 with lanes == NULL"),
                            ((0, None, 0, 0, B, L, sd, Q, lv.ctypes.data, NR, lm.ctypes.data, None, None, None, None), "are all NULL"),
                            ((0, None, 0, 0, B, L, sd, 0, None, 0, None, None, out.ctypes.data, out.ctypes.data, None), "are all NULL"),
                            ((0, None, 0, 0, B, L, sd, 0, None, 0, None, out.ctypes.data, None, None, raw.ctypes.data),
                             "raw_out given in all-lanes mode")):
            assert f(e._h, *args) == -1
            assert re.search(named, D.lib().bt_last_error().decode()), D.lib().bt_last_error().decode()
        assert f(None, 0, None, 0, 0, B, L, sd, 0, None, 0, None, out.ctypes.data, None, None, None) == -1
        assert "null engine" in D.lib().bt_last_error().decode()
        assert f(e._h, 0, None, 0, 0, B, L, sd, 0, None, 0, None, out.ctypes.data, None, None, None) == 0   # the records alone
        assert out.tobytes() == want.lanes.tobytes()
        with pytest.raises(D.BtError, match=r"d\[1\]\[2\] = -2147483648 outside the domain"):
            e.drawdown_of([[0, 1, 2], [3, 4, -2**31]], 5, 2)
        for d, named in ((np.zeros((0, 4), np.int64), r"n = 0 outside"), (np.zeros((2, 0), np.int64), r"T = 0 bars")):
            with pytest.raises(D.BtError, match=named):
                e.drawdown_of(d, 5, 2)
        with pytest.raises(D.BtError, match=r"mode = 3 outside \[0, 2\]"):
            e.set_ddboot_row(3)
        with pytest.raises(D.BtError, match="bytes = -1 is negative"):
            e.set_ddboot_budget(-1)
        e.set_ddboot_budget(2000)
        with pytest.raises(D.BtError, match=r"the call needs \d+ bytes of device staging, above the budget of 2000 bytes"):
            e.drawdown_risk(None, B, L, sd)
        e.set_ddboot_budget(0)
        R.assert_same(e.drawdown_risk(None, B, L, sd, None, LEVELS, LIMITS), want, "after the refusals", raw=False)
