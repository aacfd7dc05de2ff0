"""Walk-forward evaluation on the GPU (bt_walk_forward, k_walkfwd.hip; Engine.walk_forward): every
lane's fold records, the per-symbol steps and the totals, bit for bit against the reference of
walkfwd_ref.py (C oracle trade lists, Python-int sums; pinned to the oracle in
test_walkfwd_cpu.py), equal to the sweep where one fold is the whole series, and independent of how
the rows are chunked through the device staging."""
import re

import numpy as np
import pytest

import dbx_amd as D
from dbx_amd import engine as E
import walkfwd_ref as R
from replay_ref import gen_hlc

pytestmark = pytest.mark.gpu

STRATEGIES = ("sma", "ema_ols", "boll")


def _load(e, strategy, series, ids=None):
    """series: [(h, l, c)]"""
    if strategy == "boll":
        e.load_ohlc([s[2] for s in series], [s[0] for s in series], [s[1] for s in series], sym_ids=ids)
    else:
        e.load_ohlc([s[2] for s in series], sym_ids=ids)


# ------------------------------------------------------------------------------------- edges
@pytest.mark.parametrize("strategy", STRATEGIES)
def test_edges_every_lane_every_fold_bit_exact(strategy):
    grid, folds, _ = R.edge_case(strategy)
    assert grid.n_params == 12 and folds.shape == (9, 12, 10)
    traded, open_end, exit_last, entry_first = R.edge_counts(strategy)
    assert traded >= 30 and open_end >= 15 and exit_last >= 3 and entry_first >= 3
    with D.Engine(grid) as e:
        _load(e, strategy, R.edge_series(), R.EDGE_IDS)
        got = {train: e.walk_forward(R.EDGE_BOUNDS, train=train, folds=True) for train in (0, 1, 3)}   # no run()
    for train, wf in got.items():
        steps, total, _ = R.ref_steps(folds, R.EDGE_IDS, train, grid.annualization)
        assert wf.folds.dtype == D.FOLD_DTYPE and wf.steps.shape == (9, 10 - max(train, 1))
        R.assert_same(wf.folds, folds, f"{strategy} folds, train {train}")
        R.assert_same(wf.steps, steps, f"{strategy} steps, train {train}")
        R.assert_same(wf.total, total, f"{strategy} totals, train {train}")
        assert (steps["param"] >= 0).any() and (steps["param"] < 0).any()


# --------------------------------------------------------------------- one fold is the sweep
PRODUCT = {
    "config2": (D.config2_grid, 16, 2520, D.BT_DAILY),
    "config3": (D.config3_grid, 4, 6000, D.BT_MINUTE),
    "config4": (D.config4_grid, 4, 6000, D.BT_MINUTE),
}


@pytest.mark.parametrize("name", list(PRODUCT))
def test_one_fold_equals_the_sweep_and_leaves_it_alone(name):
    mk, n_sym, bars, freq = PRODUCT[name]
    grid = mk()
    with D.Engine(grid, topk=32) as e:
        e.load_synthetic(0xD1CE, 1000, n_sym, bars, freq)
        e.run()
        before = (e.summaries().copy(), e.read_topk().copy(), e.stats(), e.last_segments(with_refixed=True))
        wf = e.walk_forward((0, bars), train=0, folds=True)
        after = (e.summaries().copy(), e.read_topk().copy(), e.stats(), e.last_segments(with_refixed=True))
    summ = before[0]
    assert wf.folds.shape == (n_sym, grid.n_params, 1) and wf.steps.shape == (n_sym, 0)
    f = wf.folds[:, :, 0]
    assert (f["first_bar"] == 0).all() and (f["n_bars"] == bars).all() and (f["status"] == 0).all()
    for name_ in ("pnl", "mdd", "exposure", "n_trades"):
        bad = np.argwhere(f[name_].astype(np.int64) != summ[name_].astype(np.int64))
        assert not len(bad), f"{name}: {name_} differs first at (sym, param) {bad[:1]}"
    bad = np.argwhere(f["sharpe"].view(np.uint64) != summ["sharpe"].view(np.uint64))
    assert not len(bad), f"{name}: sharpe differs first at (sym, param) {bad[:1]}"
    assert int(summ["n_trades"].sum()) >= 1000
    assert before[0].tobytes() == after[0].tobytes()
    assert before[1].tobytes() == after[1].tobytes()
    assert before[2] == after[2] and before[3] == after[3]


# ----------------------------------------------------------------------- selection with ties
def test_selection_with_real_ties():
    grid, folds, _ = R.selection_case()
    with D.Engine(grid) as e:
        e.load_synthetic(R.SEL_SEED, R.SEL_IDS[0], len(R.SEL_IDS), R.SEL_BARS, D.BT_DAILY)
        got = {train: e.walk_forward(R.SEL_BOUNDS, train=train, folds=train == 1) for train in (0, 1, 2)}
    R.assert_same(got[1].folds, folds, "selection folds")
    assert got[0].folds is None
    for train, wf in got.items():
        steps, total, tied = R.selection_steps(train)
        picks = steps["param"][steps["param"] >= 0]
        assert len(np.unique(picks)) >= 15 and sum(n > 1 for row in tied for n in row) >= 5
        R.assert_same(wf.steps, steps, f"steps, train {train}")
        R.assert_same(wf.total, total, f"totals, train {train}")
        assert np.array_equal(wf.oos_sharpe().view(np.uint64), total["sharpe"].view(np.uint64))
        assert np.array_equal(wf.train_sharpe().view(np.uint64), steps["train_sharpe"].view(np.uint64))
        assert set(grid.param(int(picks[0]))) == {"f", "s"}


# ------------------------------------------------------------------------------------ chunks
def test_chunking_is_invisible():
    """The same calls with the staging budget forced to one row (selection shape) and to three
    rows (edge shape) per chunk: the outputs are the bytes of the one-chunk call."""
    grid, folds, _ = R.selection_case()
    with D.Engine(grid) as e:
        e.load_synthetic(R.SEL_SEED, R.SEL_IDS[0], len(R.SEL_IDS), R.SEL_BARS, D.BT_DAILY)
        whole = e.walk_forward(R.SEL_BOUNDS, train=2, folds=True)
        e.set_walkfwd_budget(6 * 400 * 80 + 4096)        # one row's records and steps, not two
        one = e.walk_forward(R.SEL_BOUNDS, train=2, folds=True)
        only_total = E.sym("bt_walk_forward")
        total = np.zeros(6, D.FOLD_DTYPE)
        b = np.asarray(R.SEL_BOUNDS, np.int32)
        assert only_total(e._h, 6, b.ctypes.data, 2, None, None, total.ctypes.data) == 0
        e.set_walkfwd_budget(0)
        again = e.walk_forward(R.SEL_BOUNDS, train=2, folds=True)
    for wf, what in ((one, "one row per chunk"), (again, "default budget again")):
        R.assert_same(wf.folds, whole.folds, f"folds, {what}")
        R.assert_same(wf.steps, whole.steps, f"steps, {what}")
        R.assert_same(wf.total, whole.total, f"totals, {what}")
    R.assert_same(total, whole.total, "total alone, one row per chunk")
    R.assert_same(whole.folds, folds, "folds")
    egrid, efolds, _ = R.edge_case("boll")
    with D.Engine(egrid) as e:
        _load(e, "boll", R.edge_series(), R.EDGE_IDS)
        whole = e.walk_forward(R.EDGE_BOUNDS, train=1, folds=True)
        e.set_walkfwd_budget(40000)                      # three rows of 12 x 10 records
        three = e.walk_forward(R.EDGE_BOUNDS, train=1, folds=True)
    R.assert_same(three.folds, whole.folds, "edge folds, three rows per chunk")
    R.assert_same(three.steps, whole.steps, "edge steps, three rows per chunk")
    R.assert_same(three.total, whole.total, "edge totals, three rows per chunk")
    R.assert_same(whole.folds, efolds, "edge folds")


# ---------------------------------------------------------------------------------- refusals
def test_refusals_name_the_value_and_leave_the_engine_usable():
    grid, folds, _ = R.edge_case("sma")
    want_steps, want_total, _ = R.ref_steps(folds, R.EDGE_IDS, 1, grid.annualization)

    def still_good(e):
        wf = e.walk_forward(R.EDGE_BOUNDS, train=1, folds=True)
        R.assert_same(wf.folds, folds, "folds after a refusal")
        R.assert_same(wf.steps, want_steps, "steps after a refusal")
        R.assert_same(wf.total, want_total, "totals after a refusal")

    with D.Engine(grid) as e:
        with pytest.raises(D.BtError, match="no dataset"):
            e.walk_forward((0, 10, 20))
        _load(e, "sma", R.edge_series(), R.EDGE_IDS)
        still_good(e)
        for bounds, kw, named in (
            ((5,), {}, r"K = 0 "),
            ((0, 10, 10, 20), {}, r"bounds\[2\] = 10 does not exceed bounds\[1\] = 10"),
            ((0, 30, 20), {}, r"bounds\[2\] = 20 does not exceed bounds\[1\] = 30"),
            ((-1, 10, 20), {}, r"bounds\[0\] = -1 "),
            ((0, 10, 20), {"train": 2}, r"train = 2 outside \[0, 1\]"),
            ((0, 10, 20), {"train": -1}, r"train = -1 "),
        ):
            with pytest.raises(D.BtError, match=named):
                e.walk_forward(bounds, **kw)
            still_good(e)
        e.set_walkfwd_budget(1000)
        with pytest.raises(D.BtError, match=r"P\*K = 12\*10 records of one row exceed the staging budget of 1000 bytes"):
            e.walk_forward(R.EDGE_BOUNDS)
        with pytest.raises(D.BtError, match="bytes = -5 "):
            e.set_walkfwd_budget(-5)
        e.set_walkfwd_budget(0)
        still_good(e)
        # the raw binding: outputs that do not fit the call
        f = E.sym("bt_walk_forward")
        one = np.asarray((0, 1000), np.int32)
        two = np.asarray((0, 500, 1000), np.int32)
        many = np.arange(40000, dtype=np.int32)          # 9 * 12 * 39,999 records > 2^22
        steps = np.zeros((9, 2), D.WF_STEP_DTYPE)
        total = np.zeros(9, D.FOLD_DTYPE)
        rec = np.zeros(9 * 12 * 2, D.FOLD_DTYPE)
        for args, named in (
            ((1, one.ctypes.data, 0, None, steps.ctypes.data, None), r"K = 1: steps and total need at least 2 folds"),
            ((1, one.ctypes.data, 0, None, None, total.ctypes.data), r"K = 1: steps and total"),
            ((2, two.ctypes.data, 1, None, None, None), r"folds, steps and total are all NULL"),
            ((39999, many.ctypes.data, 1, rec.ctypes.data, None, None), r"S\*P\*K = 9\*12\*39999 exceeds 2\^22"),
            ((2, None, 1, rec.ctypes.data, None, None), r"bounds are required"),
        ):
            assert f(e._h, *args) == -1
            msg = D.lib().bt_last_error().decode()
            assert re.search(named, msg), msg
            still_good(e)
        assert f(e._h, 2, two.ctypes.data, 1, rec.ctypes.data, steps.ctypes.data, total.ctypes.data) == 0
        with pytest.raises(D.BtError, match=r"exceeds 2\^22"):
            e.walk_forward(many, folds=True)
        still_good(e)


# -------------------------------------------------------------------------------- short rows
@pytest.mark.parametrize("strategy", STRATEGIES)
def test_short_rows_have_no_steps_and_the_totals_skip_them(strategy):
    grid = R.EDGE_GRIDS[strategy]()
    ids, bars = (7, 300, 8, 9), (65, 1000, 1000, 65)
    series = [gen_hlc(0x5407, i, b, 1) for i, b in zip(ids, bars)]
    short = [i for i, b in enumerate(bars) if b == 65]
    for bounds in ((100, 300, 500, 700, 1000), (0, 60, 64, 65, 400, 1000)):
        folds, _ = R.ref_folds(strategy, grid, series, bounds)
        steps, total, _ = R.ref_steps(folds, ids, 1, grid.annualization)
        with D.Engine(grid) as e:
            _load(e, strategy, series, ids)
            wf = e.walk_forward(bounds, train=1, folds=True)
        R.assert_same(wf.folds, folds, f"{strategy} folds {bounds}")
        R.assert_same(wf.steps, steps, f"{strategy} steps {bounds}")
        R.assert_same(wf.total, total, f"{strategy} totals {bounds}")
        past = [j for j in range(1, len(bounds) - 1) if bounds[j] >= 65]   # steps whose fold the short rows lack
        assert past
        for s in short:
            st = wf.steps[s][[j - 1 for j in past]]
            assert (st["param"] == -1).all() and not st["train_sharpe"].any() and (st["sym"] == ids[s]).all()
            assert (st["oos"]["first_bar"] == 65).all()
            blank = st["oos"].copy()
            blank["first_bar"] = 0
            assert not blank.view(np.uint8).any(), "oos of a step without a fold is the empty record"
        if bounds[0] >= 65:
            assert not wf.total[short].view(np.uint8).any(), "totals of rows without a step are zero"
            assert (wf.folds[short]["first_bar"] == 65).all() and not wf.folds[short]["n_bars"].any()
        long = [i for i in range(len(bars)) if i not in short]
        assert (wf.steps[long]["param"] >= 0).all() and (wf.total[long]["n_bars"] > 0).all()
