"""The probability of backtest overfitting on the GPU (bt_cscv / bt_cscv_of, k_cscv.hip;
Engine.cscv): group counts, histograms and every combination's pick, byte for byte against the
Python-int reference of cscv_ref.py or, on shapes too large for it, against bt_cscv_host, which
test_cscv_cpu.py pins to that reference; independent of how the rows are chunked and of how the
launch cap cuts a row's pairs; the walked form equal to the staged form on the walk's own records."""
import numpy as np
import pytest

import cscv_ref as R
import dbx_amd as D
import walkfwd_ref as W
from dbx_amd import engine as E
from test_cscv_cpu import crafted_ref, edge_ref, same

pytestmark = pytest.mark.gpu

STRATEGIES = ("sma", "ema_ols", "boll")
REF_CELLS = 200_000      # (lane, combination) cells up to which the Python reference is the yardstick


def _load(e, strategy, series, ids=None):
    if strategy == "boll":
        e.load_ohlc([s[2] for s in series], [s[0] for s in series], [s[1] for s in series], sym_ids=ids)
    else:
        e.load_ohlc([s[2] for s in series], sym_ids=ids)


def _one_row_budget(P, K, picks=True):
    """A staging budget that holds one row of the call and not two (csrc/plan.cpp plan_cscv)."""
    C = len(R.masks(K))
    row = K * P * 80 + P * (K + 1) * 32 + K * 4 + 32 + (2 * P - 1) * 4 + (C * 24 if picks else 0)
    fixed = 256 + -(-(C // 2 * 4) // 256) * 256 + 6 * 256
    return fixed + row + row // 2


def _bytes(o):
    return o.groups.tobytes(), o.hist.tobytes(), o.picks.tobytes()


@pytest.fixture(scope="module")
def bare():
    """An engine without a dataset: all the staged form needs."""
    with D.Engine(D.Grid.sma([3], [5])) as e:
        yield e


# ------------------------------------------------------------------------------------- 1. edges
@pytest.mark.parametrize("strategy", STRATEGIES)
def test_edges_equal_the_reference_whatever_the_chunks_and_launches(strategy):
    grid, folds, _ = W.edge_case(strategy)
    with D.Engine(grid, topk=8) as e:
        _load(e, strategy, W.edge_series(), W.EDGE_IDS)
        e.run()
        before = (e.summaries().copy(), e.read_topk().copy(), e.stats())
        whole = e.cscv(W.EDGE_BOUNDS, hist=True, picks=True)
        e.set_walkfwd_budget(_one_row_budget(12, 10))
        e.set_cscv_work(12 * 40)             # 126 pairs of a row in launches of 40: four per row
        cut = e.cscv(W.EDGE_BOUNDS, hist=True, picks=True)
        e.set_cscv_work(1)                   # one pair per launch
        e.set_walkfwd_budget(0)
        single = e.cscv(W.EDGE_BOUNDS, hist=True, picks=False)
        after = (e.summaries().copy(), e.read_topk().copy(), e.stats())
    same(whole, edge_ref(strategy), strategy)
    assert _bytes(cut) == _bytes(whole)
    assert single.picks is None and single.groups.tobytes() == whole.groups.tobytes()
    assert single.hist.tobytes() == whole.hist.tobytes()
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
    assert before[2] == after[2]
    assert whole.groups["sym"].tolist() == list(W.EDGE_IDS)


# ------------------------------------------------------------------------- 2. the selection shape
def test_selection_shape_walked_equals_staged_equals_host():
    grid, folds, _ = W.selection_case()
    assert grid.n_params == 400 and folds.shape == (6, 400, 6)
    host = D.cscv_host(folds, W.SEL_IDS, grid.annualization, hist=True, picks=True)
    assert int(host.groups["n_tied"].sum()) > 0 and int(host.groups["n_live"].sum()) == 6 * 20
    with D.Engine(grid) as e:
        e.load_synthetic(W.SEL_SEED, W.SEL_IDS[0], len(W.SEL_IDS), W.SEL_BARS, D.BT_DAILY)
        walked = e.cscv(W.SEL_BOUNDS, hist=True, picks=True)
        wf = e.walk_forward(W.SEL_BOUNDS, folds=True)
        staged = e.cscv(folds=wf.folds, sym_ids=W.SEL_IDS, hist=True, picks=True)
        e.set_walkfwd_budget(_one_row_budget(400, 6))
        chunked = e.cscv(W.SEL_BOUNDS, hist=True, picks=True)
    W.assert_same(wf.folds, folds, "selection folds")
    same(walked, (host.groups, host.hist, host.picks), "walked against the host")
    assert _bytes(staged) == _bytes(walked) and _bytes(chunked) == _bytes(walked)
    assert walked.pbo().shape == (6,) and ((walked.pbo() >= 0) & (walked.pbo() <= 1)).all()


# ---------------------------------------------------------------------------- 3. crafted records
SHAPES = [(K, P, 3) for K in (2, 4, 16) for P in (1, 2, 3, 64, 65, 257)] + [(20, 3, 1)]


@pytest.mark.parametrize("K,P,G", SHAPES)
def test_crafted_records_through_the_staged_form(bare, K, P, G):
    f = R.crafted(K, P, G, 11)
    C = len(R.masks(K))
    picks = G * C <= D.CSCV_PICKS_MAX
    ids = [1000 + 7 * g for g in range(G)]
    if P * C * G <= REF_CELLS:
        want = R.ref_cscv(f, ids, bare.grid.annualization)
    else:
        h = D.cscv_host(f, ids, bare.grid.annualization, hist=True, picks=True)
        want = (h.groups, h.hist, h.picks)
    got = bare.cscv(folds=f, sym_ids=ids, hist=True, picks=picks)
    same(got, want, f"K={K} P={P}")
    assert (got.groups["n_live"] + got.groups["n_dead"] == C).all()
    if G > 1:      # folds without return bars in group 1, bars in bit K - 1's fold only in the last
        assert got.groups[-1]["n_dead"] == C
        assert 0 < got.groups[1]["n_dead"] or K == 2
    if (K, P) in ((16, 65), (4, 257), (2, 3)):    # the launch cap cuts rows and pairs: the same bytes
        bare.set_cscv_work(P * 100)
        bare.set_walkfwd_budget(_one_row_budget(P, K) + (K * P * 112 + C * 24))   # two rows a chunk
        try:
            cut = bare.cscv(folds=f, sym_ids=None, hist=True, picks=picks)
        finally:
            bare.set_cscv_work(0)
            bare.set_walkfwd_budget(0)
        assert cut.groups["sym"].tolist() == list(range(G))
        cut.groups["sym"] = ids
        assert _bytes(cut) == _bytes(got)


def test_refusals_leave_the_engine_usable(bare):
    f = R.crafted(4, 3, 2, 11)
    with pytest.raises(D.BtError, match="bt_cscv: no dataset loaded"):
        bare.cscv((0, 10, 20))
    bad = f.copy()
    bad[1, 2, 3]["n_bars"] += 1
    with pytest.raises(D.BtError, match=r"bt_cscv_of: first_bar, n_bars = .* \(group 1, lane 2, fold 3\)"):
        bare.cscv(folds=bad)
    with pytest.raises(D.BtError, match="bt_cscv_of: K = 3 is odd"):
        bare.cscv(folds=f[:, :, :3])
    with pytest.raises(D.BtError, match="bt_set_cscv_work: cells = -1 is negative"):
        bare.set_cscv_work(-1)
    bare.set_walkfwd_budget(1)
    try:
        with pytest.raises(D.BtError, match="bt_cscv_of: one row of P = 3 lanes and K = 4 folds needs .* above the staging budget of 1"):
            bare.cscv(folds=f)
    finally:
        bare.set_walkfwd_budget(0)
    assert len(bare.cscv(folds=f[:0]).groups) == 0
    want = R.ref_cscv(f, None, bare.grid.annualization)
    same(bare.cscv(folds=f, hist=True, picks=True), want, "after the refusals")
    with D.Engine(D.Grid.sma([3, 4], [5, 9])) as e:
        e.load_synthetic(1, 0, 2, 100, D.BT_DAILY)
        for bounds, named in (((0, 10, 20, 30), "K = 3 is odd"), ((0, 10, 10), r"bounds\[2\] = 10 does not exceed"),
                              ((-1, 10, 20), r"bounds\[0\] = -1 is negative"), ((0,), r"K = 0 outside \[2, 20\]")):
            with pytest.raises(D.BtError, match="bt_cscv: " + named):
                e.cscv(bounds)
        assert E.sym("bt_cscv")(e._h, 2, np.array([0, 50, 100], np.int32).ctypes.data, None, None, None) == -1
        assert "groups, hist and picks are all NULL" in D.lib().bt_last_error().decode()
        assert e.cscv((0, 50, 100)).groups["n_live"].tolist() == [2, 2]


# ---------------------------------------------------------------------------- 4. derived figures
def test_derived_figures_from_the_reference_records():
    grid, folds, _ = W.edge_case("sma")
    groups, hist, picks = edge_ref("sma")
    with D.Engine(grid) as e:
        _load(e, "sma", W.edge_series(), W.EDGE_IDS)
        o = e.cscv(W.EDGE_BOUNDS, hist=True, picks=True)
    live = groups["n_live"].tolist()
    assert o.pbo().tolist() == [a / b if b else 0.0 for a, b in zip(groups["n_overfit"].tolist(), live)]
    assert o.prob_loss().tolist() == [a / b if b else 0.0 for a, b in zip(groups["n_loss"].tolist(), live)]
    assert o.pbo()[0] == 0.0 and o.pbo().max() > 0       # the one-bar row: every combination dead
    assert o.omega().tolist() == [(r2 + 2) / 26 for r2 in range(23)]
    assert (o.combos == np.array(R.masks(10), np.uint32)).all()
    d = o.degradation()
    for g in range(9):
        pk = picks[g][picks[g]["lane"] >= 0]
        x, y = pk["is_sharpe"], pk["oos_sharpe"]
        if len(pk) and np.ptp(x) > 0:
            dx = x - x.mean()
            slope = float(dx @ (y - y.mean())) / float(dx @ dx)
            assert d[g].tolist() == [slope, y.mean() - slope * x.mean()]
        else:
            assert d[g].tolist() == [0.0, 0.0]
    assert np.abs(d).max() > 0
