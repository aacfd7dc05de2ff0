"""Covariance of chosen lanes on the GPU (bt_covariance, bt_gram_of, k_gram.hip; Engine.covariance):
the Gram matrix, the sums and T bit for bit against the reference of gram_ref.py (C oracle trade
lists, Python-int sums; test_gram_cpu.py holds bt_covariance_host to the same reference), crafted
increment matrices that isolate every term of the 16-bit split and reach the top of the exactness
bound, and the properties the spec states: independent of the bar chunks, additive over windows,
and the portfolio's s1 and s2 when summed."""
import re

import numpy as np
import pytest

import dbx_amd as D
from dbx_amd import engine as E
import gram_ref as G
import walkfwd_ref as R

pytestmark = pytest.mark.gpu

STRATEGIES = ("sma", "ema_ols", "boll")


def _load(e, strategy, series, ids=None):
    """series: [(h, l, c)]"""
    if strategy == "boll":
        e.load_ohlc([s[2] for s in series], [s[0] for s in series], [s[1] for s in series], sym_ids=ids)
    else:
        e.load_ohlc([s[2] for s in series], sym_ids=ids)


def _i128(r):
    return (int(r["hi"]) << 64) | int(r["lo"])


# ------------------------------------------------------------------------------------- 1. edges
@pytest.mark.parametrize("strategy", STRATEGIES)
def test_edges_gram_sums_and_T_bit_exact(strategy):
    grid, lanes, curves = G.edge_lanes(strategy)
    assert len(lanes) == 21 and len(set(lanes)) == 20
    with D.Engine(grid) as e:
        _load(e, strategy, R.edge_series(), R.EDGE_IDS)
        got = {w: e.covariance(lanes, w) for w in G.WINDOWS}   # no run()
        default = e.covariance(lanes)
        rp = e.replay(lanes, curves=True)
    for w, cv in got.items():
        assert cv.wide.dtype == D.WIDE_DTYPE and cv.wide.shape == (21, 21)
        G.assert_equal(cv, G.edge_reference(strategy, w), f"{strategy} window {w}")
    G.assert_equal(default, G.edge_reference(strategy, (0, G.WHOLE)), f"{strategy}, no window")
    assert got[(5, 5)].n_bars == 0 and not got[(5, 5)].wide.tobytes().strip(b"\0") and not got[(5, 5)].sums.any()
    # short symbols contribute zeros after their end
    tail = got[(500, 1000)]
    short = [k for k, c in enumerate(curves) if len(c) <= 500]
    assert len(short) >= 16 and not tail.wide[short].tobytes().strip(b"\0") and not tail.sums[short].any()
    # the diagonal is the sum of squares of the lane's replayed curve
    for i in range(21):
        eq = [int(x) for x in rp.equity[i][:int(rp.n_bars[i])]]
        d = [b - a for a, b in zip([0] + eq[:-1], eq)]
        assert _i128(default.wide[i, i]) == sum(x * x for x in d) and int(default.sums[i]) == sum(d), f"lane {i}"
    assert np.array_equal(default.wide, default.wide.T), "symmetric"


# --------------------------------------------------------------------------- 2. crafted gram_of
@pytest.fixture(scope="module")
def bare():
    """An engine without a dataset: gram_of needs none."""
    with D.Engine(D.Grid.sma([2], [5])) as e:
        yield e


@pytest.mark.parametrize("name", ("low", "high", "half", "ends"))
def test_gram_of_isolates_every_term_of_the_split(bare, name):
    d = G.crafted(name)
    assert d.shape == (20, 67)
    a = d.astype(np.int64)
    if name == "low":
        assert np.abs(a).max() < 2**15
    elif name == "high":
        assert not (a % 65536).any() and np.abs(a).max() >= 2**30
    elif name == "half":
        assert ((a % 65536) == 0x8000).all() and a.max() == 0x7FFF8000
    else:
        assert (np.abs(a) == 2**31 - 1).all() and (a > 0).any() and (a < 0).any()
    G.assert_equal(bare.gram_of(d), G.gram_of_reference(d), name)


@pytest.mark.parametrize("T", (1, 3, 63, 64, 65))
def test_gram_of_random_full_range(bare, T):
    """n = 33: three tile rows with a ragged last one; every entry distinct, so a wrong fragment
    map (a transposed tile, the f32 row formula, A and B reading different bars) cannot pass."""
    d = G.crafted("full", 33, T, seed=T)
    got = bare.gram_of(d)
    G.assert_equal(got, G.gram_of_reference(d), f"full T {T}")
    assert np.array_equal(got.wide, got.wide.T)


def test_gram_of_the_top_of_the_bound(bare):
    """n = 2, T = 2^22, every d = 2^31 - 1: the HH accumulator ends at 2^22 * 2^30 = 2^52."""
    T, v = 1 << 22, 2**31 - 1
    d = np.full((2, T), v, np.int32)
    got = bare.gram_of(d)
    G.assert_equal(got, G.constant_gram(2, T, v), "top of the bound")
    assert int(got.gram[0, 1]) == (1 << 22) * v * v > 2**83
    d[1] = -v
    d[1, ::2] = 0x7FFF8000   # h = 2^15, l = -2^15 on half the bars
    got = bare.gram_of(d)
    half = T // 2
    want = np.empty((2, 2), object)
    want[0, 0] = T * v * v
    want[0, 1] = want[1, 0] = half * v * 0x7FFF8000 - half * v * v
    want[1, 1] = half * 0x7FFF8000**2 + half * v * v
    G.assert_equal(got, (want, np.array([T * v, half * 0x7FFF8000 - half * v], np.int64), T), "mixed ends")


# ------------------------------------------------------------------------- 3. split invariance
def test_split_invariance(bare):
    d = G.crafted("full", 33, 1000, seed=1000)
    want = G.gram_of_reference(d)
    out = {}
    try:
        for k in (1, 2, 7, 0):
            bare.set_gram_split(k)
            out[k] = bare.gram_of(d)
    finally:
        bare.set_gram_split(0)
    for k, cv in out.items():
        G.assert_equal(cv, want, f"split {k}")
        assert cv.wide.tobytes() == out[1].wide.tobytes() and cv.sums.tobytes() == out[1].sums.tobytes()


# ------------------------------------------------------- 4. additivity, 5. against bt_portfolio
def test_windows_add_and_the_sums_are_the_portfolio_s():
    grid = D.config2_grid()
    lanes = [(300 + s, (37 * k + 11 * s) % grid.n_params) for s in range(6) for k in range(4)]
    assert len(lanes) == 24
    with D.Engine(grid) as e:
        e.load_synthetic(0xC0FE, 300, 6, 600, D.BT_DAILY)
        whole = e.covariance(lanes, (0, 600))
        parts = {a: (e.covariance(lanes, (0, a)), e.covariance(lanes, (a, 600))) for a in (1, 64, 333)}
        pf = e.portfolio(lanes)
        rp = e.replay(lanes, curves=True)
    assert whole.n_bars == 600 and whole.sums.any()
    for a, (lo, hi) in parts.items():
        assert (lo.n_bars, hi.n_bars) == (a, 600 - a)
        assert np.array_equal(lo.gram + hi.gram, whole.gram), f"cut at {a}"
        assert np.array_equal(lo.sums + hi.sums, whole.sums), f"cut at {a}"
    s = pf.summary
    assert int(s["n_bars"]) == 600 and int(s["n_lanes"]) == 24
    assert whole.book_s2() == (int(s["s2_hi"]) << 64) | int(s["s2_lo"])
    assert int(whole.sums.sum()) == (int(s["s1_hi"]) << 64) | int(s["s1_lo"]) == int(s["pnl"])
    # and the host restatement from the replayed curves gives the same bytes
    host = D.covariance_host(rp.equity, rp.n_bars, (0, 600))
    assert host.wide.tobytes() == whole.wide.tobytes() and np.array_equal(host.sums, whole.sums)


# --------------------------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_engine_usable_and_the_run_alone():
    grid, lanes, _ = G.edge_lanes("sma")
    want = G.edge_reference("sma", (64, 128))
    with D.Engine(grid, topk=16) as e:
        with pytest.raises(D.BtError, match="bt_covariance: no dataset"):
            e.covariance([(0, 0)])
        _load(e, "sma", R.edge_series(), R.EDGE_IDS)
        e.run()
        before = (e.summaries().copy(), e.read_topk().copy(), e.stats(), e.last_segments(with_refixed=True))
        G.assert_equal(e.covariance(lanes, (64, 128)), want, "after run()")
        top = e.read_topk().copy()
        G.assert_equal(e.covariance(top, (0, 50)), _replayed(e, top, (0, 50)), "top-k records feed straight in")
        after = (e.summaries().copy(), top, e.stats(), e.last_segments(with_refixed=True))
        assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
        assert before[2] == after[2] and before[3] == after[3] and len(top) == 16
        e.run()
        assert e.summaries().tobytes() == before[0].tobytes() and e.read_topk().tobytes() == before[1].tobytes()

        def bad(i, lane):
            a = list(lanes)
            a[i] = lane
            return a

        for req, window, named in (
            (bad(5, (123456, 0)), (0, 10), r"unknown symbol id 123456 \(lane 5\)"),
            (bad(9, (650, 12)), (0, 10), r"param 12 outside \[0, 12\) \(lane 9\)"),
            (bad(9, (650, -1)), (0, 10), r"param -1 outside"),
            (lanes, (-2, 10), r"from_bar = -2 is negative"),
            (lanes, (50, 49), r"to_bar = 49 is below from_bar = 50"),
            ([(650, 0)] * 2049, (0, 10), r"n = 2049 outside \[0, 2048\]"),
        ):
            with pytest.raises(D.BtError, match=named):
                e.covariance(req, window)
            G.assert_equal(e.covariance(lanes, (64, 128)), want, f"after the refusal {named}")
        f, g = E.sym("bt_covariance"), E.sym("bt_gram_of")
        req = D.as_lanes(lanes)
        wide, sums, T = np.zeros(21 * 21, D.WIDE_DTYPE), np.zeros(21, np.int64), np.zeros(1, np.int32)
        out = (wide.ctypes.data, sums.ctypes.data, T.ctypes.data)
        d = np.arange(12, dtype=np.int32).reshape(3, 4)
        d[2, 1] = -2**31
        for call, args, named in (
            (f, (-1, req.ctypes.data, 0, 10, *out), r"bt_covariance: n = -1 outside \[0, 2048\]"),
            (f, (21, None, 0, 10, *out), r"lanes are required"),
            (f, (21, req.ctypes.data, 0, 10, None, None, None), r"gram, sums and T are all NULL"),
            (g, (-1, 4, d.ctypes.data, out[0], out[1]), r"bt_gram_of: n = -1 outside \[0, 2048\]"),
            (g, (2049, 4, d.ctypes.data, out[0], out[1]), r"n = 2049 outside"),
            (g, (3, -1, d.ctypes.data, out[0], out[1]), r"T = -1 outside \[0, 4194304\]"),
            (g, (3, (1 << 22) + 1, d.ctypes.data, out[0], out[1]), r"T = 4194305 outside"),
            (g, (3, 4, None, out[0], out[1]), r"d is required"),
            (g, (3, 4, d.ctypes.data, None, None), r"gram and sums are both NULL"),
            (g, (3, 4, d.ctypes.data, out[0], out[1]), r"d\[2\]\[1\] = -2147483648 outside the domain"),
            # 2,048 rows of 2^16 bars: 512 MB of increments alone (the rule comes before d is read)
            (g, (2048, 1 << 16, d.ctypes.data, out[0], out[1]),
             r"n = 2048 lanes over T = 65536 bars need \d+ bytes of device staging, above 268435456"),
        ):
            assert call(e._h, *args) == -1
            msg = D.lib().bt_last_error().decode()
            assert re.search(named, msg), msg
        with pytest.raises(D.BtError, match="k = -1 is negative"):
            e.set_gram_split(-1)
        G.assert_equal(e.covariance(lanes, (64, 128)), want, "after the raw refusals")
        # one output alone, and no lane at all
        only = np.zeros(1, np.int32)
        assert f(e._h, 1, req.ctypes.data, 0, 7, None, None, only.ctypes.data) == 0 and int(only[0]) == 1   # a 1-bar symbol
        assert f(e._h, 0, None, 0, 7, None, None, only.ctypes.data) == 0 and int(only[0]) == 0
        none = e.covariance([])
        assert none.n_bars == 0 and none.wide.shape == (0, 0) and none.sums.shape == (0,)
        assert e.gram_of(np.zeros((3, 0), np.int32)).n_bars == 0


def _replayed(e, top, window):
    rp = e.replay(top, curves=True)
    return G.covariance([[int(x) for x in rp.equity[i][:int(rp.n_bars[i])]] for i in range(len(top))], window)
