"""Portfolio of chosen lanes on the GPU (bt_portfolio, k_portfolio.hip; Engine.portfolio): every
per-bar row and the summary, bit for bit against the reference of portfolio_ref.py (C oracle trade
lists, Python-int sums; test_portfolio_cpu.py holds bt_portfolio_host to the same reference),
against the replay of one lane, against the walk-forward totals, and independent of the replica
count when thousands of waves add to the same bars."""
import re

import numpy as np
import pytest

import dbx_amd as D
from dbx_amd import engine as E
import portfolio_ref as PR
import walkfwd_ref as R

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
def test_edges_every_row_and_the_summary_bit_exact(strategy):
    grid, lanes, _, trades = PR.edge_entries(strategy)
    assert PR.begins_inside_a_trade(lanes, trades) >= 3
    with D.Engine(grid) as e:
        _load(e, strategy, R.edge_series(), R.EDGE_IDS)
        got = {T: e.portfolio(lanes, n_bars=T) for T in (1000, 130)}   # no run()
        default = e.portfolio(lanes)
    for T, pf in got.items():
        assert pf.summary.dtype == D.PF_SUMMARY_DTYPE and pf.pnl.shape == (T,)
        PR.assert_equal(pf, PR.edge_reference(strategy, T), f"{strategy} T {T}")
    PR.assert_equal(default, PR.edge_reference(strategy, 1000), f"{strategy}, n_bars of the longest symbol")


# ------------------------------------------------------------------------- one entry is a replay
@pytest.mark.parametrize("strategy", STRATEGIES)
def test_one_entry_over_its_series_is_that_lane_s_replay(strategy):
    grid = R.EDGE_GRIDS[strategy]()
    with D.Engine(grid) as e:
        _load(e, strategy, R.edge_series(), R.EDGE_IDS)
        for sym, p in ((650, 0), (650, 4), (8, 1), (907, 0)):
            rp = e.replay([(sym, p)], curves=True)
            pf = e.portfolio([(sym, p)], n_bars=int(rp.n_bars[0]))
            where = f"{strategy} sym {sym} param {p}"
            assert np.array_equal(pf.equity, rp.equity[0]), where
            assert np.array_equal(pf.n_long - pf.n_short, rp.pos[0].astype(np.int32)), where
            assert np.array_equal(pf.gross(), np.abs(rp.pos[0]).astype(np.int32)), where
            s = rp.summaries[0]
            assert int(pf.summary["pnl"]) == int(s["pnl"]) and int(pf.summary["mdd"]) == int(s["mdd"]), where
            assert int(pf.summary["max_gross"]) == int(np.abs(rp.pos[0]).max()) and int(pf.summary["n_lanes"]) == 1


# ------------------------------------------------------------------ the walk-forward picks as a book
@pytest.mark.parametrize("train", (1, 2))
def test_walk_forward_picks_add_up_to_the_totals(train):
    grid, _, _ = R.selection_case()
    with D.Engine(grid) as e:
        e.load_synthetic(R.SEL_SEED, R.SEL_IDS[0], len(R.SEL_IDS), R.SEL_BARS, D.BT_DAILY)
        wf = e.walk_forward(R.SEL_BOUNDS, train=train)
        lanes = D.walk_forward_lanes(wf)
        pf = e.portfolio(lanes)
    steps, total, _ = R.selection_steps(train)
    R.assert_same(wf.steps, steps, "steps")
    assert lanes.dtype == D.PF_LANE_DTYPE and len(lanes) == int((steps["param"] >= 0).sum()) == steps.size
    assert int(pf.summary["pnl"]) == int(total["pnl"].sum()) != 0
    assert int(pf.summary["exposure"]) > 0 and int(pf.summary["n_lanes"]) == len(lanes)
    j0 = max(train, 1)
    b = R.SEL_BOUNDS
    assert (int(pf.summary["first_bar"]), int(pf.summary["n_bars"])) == (b[j0], b[-1] - b[j0])
    for j in range(j0, len(b) - 1):
        assert int(pf.pnl[b[j]:b[j + 1]].sum()) == int(steps["oos"]["pnl"][:, j - j0].sum()), f"fold {j}"
    assert not pf.pnl[:b[j0]].any() and pf.gross().max() <= len(R.SEL_IDS)


# -------------------------------------------------------------------- many adders on one row
def test_many_waves_on_the_same_bars_under_any_replica_count():
    """Every lane of the config-2 grid on 16 daily symbols: 6,400 waves start at tile 0 together and
    add to the same 2,520 bars. Against bt_portfolio_host fed from two replays with curves."""
    grid = D.config2_grid()
    n_sym, bars = 16, 2520
    lanes = [(1000 + s, p) for s in range(n_sym) for p in range(grid.n_params)]
    assert len(lanes) == 6400
    with D.Engine(grid) as e:
        e.load_synthetic(0xD1CE, 1000, n_sym, bars, D.BT_DAILY)
        a, b = e.replay(lanes[:4096], curves=True), e.replay(lanes[4096:], curves=True)
        got = {}
        for r in (1, 0, 64):
            e.set_portfolio_replicas(r)
            got[r] = e.portfolio(lanes)
    want = D.portfolio_host(np.concatenate([a.equity, b.equity]), np.concatenate([a.pos, b.pos]),
                            np.concatenate([a.n_bars, b.n_bars]), annualization=grid.annualization)
    ref = (want.pnl, want.equity, want.n_long, want.n_short, want.summary)
    for r, pf in got.items():
        PR.assert_equal(pf, ref, f"replicas {r}")
    assert int(want.summary["max_gross"]) > 3000 and int(want.summary["n_lanes"]) == 6400
    assert int(np.abs(want.pnl).max()) > 2**20


# ------------------------------------------------------------------- the dataset of a batch
def test_after_a_batch_the_bars_default_to_the_longest_requested_symbol():
    """run_batch leaves its jobs resident with ids 0, 1, ..; the wrapper does not know their bars
    and asks bt_replay for those of the requested symbols."""
    import oracle_np as N
    grid = D.Grid.sma([4, 10], [20, 50])
    jobs = []
    for s, n in ((0, 300), (1, 451), (2, 90)):
        o, h, lo, c, v = N.gen(0x5EED, [s], n, 0)
        jobs.append((f"job-{s}", N.csv_bytes(o[0], h[0], lo[0], c[0], v[0], 0)))
    with D.Engine(grid) as e:
        assert [st for st, _ in e.run_batch(jobs)] == [0, 0, 0]
        for lanes, bars in (([(0, 1), (1, 2), (2, 0), (1, 2)], 451), ([(2, 3), (0, 0)], 300)):
            rp = e.replay(lanes, curves=True)
            pf = e.portfolio(lanes, windows=(7, 400))
            want = D.portfolio_host(rp.equity, rp.pos, rp.n_bars, windows=(7, 400), T=bars,
                                    annualization=grid.annualization)
            assert len(pf.pnl) == bars and int(pf.summary["n_lanes"]) == len(lanes)
            PR.assert_equal(pf, (want.pnl, want.equity, want.n_long, want.n_short, want.summary), f"lanes {lanes}")
        assert int(pf.summary["first_bar"]) == 7 and int(pf.summary["n_bars"]) == 293 and pf.pnl.any()


# --------------------------------------------------------------------------------- magnitudes
def test_magnitudes_past_one_word_on_the_device():
    grid, series, lanes, _, want = PR.magnitude_case()
    assert int(want[4]["s2_hi"]) != 0 and int(np.abs(want[0]).max()) > 2**32
    with D.Engine(grid) as e:
        _load(e, "sma", series, PR.MAG_IDS)
        PR.assert_equal(e.portfolio(lanes), want, "magnitude case")


# ------------------------------------------------------------ the call leaves the sweep alone
def test_portfolio_leaves_the_run_alone_and_refusals_leave_the_engine_usable():
    grid, lanes, _, _ = PR.edge_entries("sma")
    want = PR.edge_reference("sma", 130)
    with D.Engine(grid, topk=16) as e:
        with pytest.raises(D.BtError, match="no dataset"):
            e.portfolio([(0, 0)], n_bars=10)
        _load(e, "sma", R.edge_series(), R.EDGE_IDS)
        e.run()
        before = (e.summaries().copy(), e.read_topk().copy(), e.stats(), e.last_segments(with_refixed=True))
        PR.assert_equal(e.portfolio(lanes, n_bars=130), want, "after run()")
        after = (e.summaries().copy(), e.read_topk().copy(), e.stats(), e.last_segments(with_refixed=True))
        assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
        assert before[2] == after[2] and before[3] == after[3]

        def bad(i, **kw):
            a = lanes.copy()
            for k, v in kw.items():
                a[k][i] = v
            return a

        for req, T, named in (
            (bad(5, sym=123456), 130, r"unknown symbol id 123456 \(entry 5\)"),
            (bad(9, param=12), 130, r"param 12 outside \[0, 12\) \(entry 9\)"),
            (bad(9, param=-1), 130, r"param -1 outside"),
            (bad(30, from_bar=-2), 130, r"from_bar = -2 is negative \(entry 30\)"),
            (bad(31, from_bar=50, to_bar=49), 130, r"to_bar = 49 is below from_bar = 50 \(entry 31\)"),
            (lanes, 0, r"T = 0 outside \[1, 4194304\]"),
            (lanes, (1 << 22) + 1, r"T = 4194305 outside"),
        ):
            with pytest.raises(D.BtError, match=named):
                e.portfolio(req, n_bars=T)
            PR.assert_equal(e.portfolio(lanes, n_bars=130), want, f"after the refusal {named}")
        f = E.sym("bt_portfolio")
        bufs = E._pf_bufs(130)
        out = [b.ctypes.data for b in bufs]
        for args, named in (
            ((-1, lanes.ctypes.data, 130, *out), r"bt_portfolio: n = -1 outside \[0, 1048576\]"),
            (((1 << 20) + 1, lanes.ctypes.data, 130, *out), r"n = 1048577 outside"),
            ((len(lanes), None, 130, *out), r"lanes are required"),
            ((len(lanes), lanes.ctypes.data, 130, None, None, None, None, None), r"are all NULL"),
        ):
            assert f(e._h, *args) == -1
            msg = D.lib().bt_last_error().decode()
            assert re.search(named, msg), msg
        with pytest.raises(D.BtError, match="r = -1 is negative"):
            e.set_portfolio_replicas(-1)
        PR.assert_equal(e.portfolio(lanes, n_bars=130), want, "after the raw refusals")
        # 2^20 windows of 1,024 and 1,025 bars on a 1,100-bar row: 2^20 * 1,024.5 window bars pass 2^30
        many = np.zeros(1 << 20, D.PF_LANE_DTYPE)
        many["sym"], many["to_bar"] = 650, 1025
        many["from_bar"][::2] = 1
        e.load_ohlc([np.full(1100, 50_000, np.int32)], sym_ids=[650])
        with pytest.raises(D.BtError, match=r"above 2\^30"):
            e.portfolio(many)
        # summary alone, and no entry at all
        only = np.zeros(1, D.PF_SUMMARY_DTYPE)
        assert f(e._h, 0, None, 5, None, None, None, None, only.ctypes.data) == 0
        assert not only.tobytes().strip(b"\0")
        none = e.portfolio([], n_bars=5)
        assert len(none.pnl) == 5 and not none.pnl.any() and not none.equity.any() and not none.gross().any()
