"""Reference for the portfolio tests (tests only), written from docs/portfolio_spec.md.

An entry's pos_t and E_t come from the C oracle's complete trade list through
replay_ref.curves_from_trades; every per-bar figure and every sum is a Python int, and the Sharpe
is the spec's formula on Python floats (int -> float rounds to nearest even, no FMA). It shares
nothing with csrc/portfolio.cpp or the kernels.

The cases the CPU and the GPU tests share are built once per process and must not be modified."""
import functools
import json
import math
import os

import numpy as np

import dbx_amd as D
import walkfwd_ref as R
from replay_ref import curves_from_trades, oracle_lane

MASK = (1 << 64) - 1
WHOLE = 2**31 - 1


def portfolio(entries, T, ann):
    """entries: [(pos, eq, from_bar, to_bar)] with pos / eq the entry's curves over its own bars.
    Returns (pnl int64[T], equity int64[T], n_long int32[T], n_short int32[T], summary record)."""
    pnl, nl, ns = [0] * T, [0] * T, [0] * T
    n_lanes, lo, hi = 0, None, None
    for pos, eq, frm, to in entries:
        to = min(to, len(eq), T)
        if to <= frm:
            continue
        n_lanes += 1
        lo = frm if lo is None else min(lo, frm)
        hi = to if hi is None else max(hi, to)
        for t in range(frm, to):
            pnl[t] += int(eq[t]) - (int(eq[t - 1]) if t else 0)
            nl[t] += pos[t] > 0
            ns[t] += pos[t] < 0
    lo, hi = lo or 0, hi or 0
    equity, run = [], 0
    for x in pnl:
        run += x
        equity.append(run)
    peak = mdd = 0
    for x in equity:
        peak = max(peak, x)
        mdd = max(mdd, peak - x)
    s1, s2 = sum(pnl[lo:hi]), sum(x * x for x in pnl[lo:hi])
    summ = np.zeros(1, D.PF_SUMMARY_DTYPE)
    r = summ[0]
    r["n_lanes"], r["first_bar"], r["n_bars"] = n_lanes, lo, hi - lo
    r["max_gross"] = max(a + b for a, b in zip(nl, ns))
    r["pnl"], r["mdd"], r["exposure"] = equity[-1], mdd, sum(nl) + sum(ns)
    r["s1_lo"], r["s1_hi"], r["s2_lo"], r["s2_hi"] = s1 & MASK, s1 >> 64, s2 & MASK, s2 >> 64
    r["sharpe"] = sharpe(s1, s2, hi - lo, ann)
    return (np.array(pnl, np.int64), np.array(equity, np.int64), np.array(nl, np.int32), np.array(ns, np.int32),
            summ[0])


def sharpe(s1, s2, n, ann):
    if n < 1:
        return 0.0
    m = float(s1) / float(n)
    v = float(s2) / float(n) - m * m
    return (m / math.sqrt(v)) * math.sqrt(float(ann)) if v > 0 else 0.0


def assert_equal(got, want, what):
    """A Portfolio against the reference tuple, byte for byte."""
    for name, w in zip(("pnl", "equity", "n_long", "n_short"), want):
        g = getattr(got, name)
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {name} {g.dtype}{g.shape} vs {w.dtype}{w.shape}"
        bad = np.nonzero(g != w)[0]
        assert not len(bad), f"{what}: {name}[{bad[0]}] = {g[bad[0]]}, want {w[bad[0]]} ({len(bad)} bars differ)"
    g, w = got.summary, want[4]
    assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), f"{what}: summary\n got  {g}\n want {w}"


# ------------------------------------------------------------------------------ the edge case
# cuts at 0, 1, 63, 64, 65 and 128, an empty window, one past every series, one reaching past them
WINDOWS = ((0, 1), (1, 63), (63, 64), (64, 65), (65, 128), (128, WHOLE), (0, 64), (5, 5), (2000, 3000),
           (10, 5000), (100, 700), (300, 999))


MID_WINDOWS = ((250, 600), (500, WHOLE), (777, 900), (420, 421))


@functools.lru_cache(None)
def edge_entries(strategy):
    """(grid, lanes PF_LANE_DTYPE[n], curves [(pos, eq)] per entry, trades per entry) on the
    walk-forward edge set (walkfwd_ref.edge_series: 9 symbols of 1 to 1,000 bars, 12 params): every
    lane over its whole series, every lane again under one of WINDOWS, the longest row's lanes under
    MID_WINDOWS, and three entries twice."""
    grid, _, lanes = R.edge_case(strategy)
    req, curves, trades = [], [], []
    series = R.edge_series()
    cache = {}

    def add(s, p, frm, to):
        if (s, p) not in cache:
            tr = lanes[s][p][1]
            pos, eq = curves_from_trades(series[s][2], tr)
            cache[s, p] = (pos.tolist(), eq.tolist(), [] if tr is None else
                           [(int(t["entry_bar"]), int(t["exit_bar"])) for t in tr])
        req.append((R.EDGE_IDS[s], p, frm, to))
        curves.append(cache[s, p][:2])
        trades.append(cache[s, p][2])

    k = 0
    for s in range(len(series)):
        for p in range(grid.n_params):
            add(s, p, 0, WHOLE)
            add(s, p, *WINDOWS[k % len(WINDOWS)])
            k += 5   # coprime with len(WINDOWS): every row meets every window
    for p in range(grid.n_params):   # more windows that begin mid-series on the 1,000-bar row
        add(8, p, *MID_WINDOWS[p % len(MID_WINDOWS)])
    for s, p in ((8, 0), (8, 5), (6, 3)):
        add(s, p, 100, 700)
        add(s, p, 100, 700)
    arr = np.zeros(len(req), D.PF_LANE_DTYPE)
    for i, r in enumerate(req):
        arr[i] = r
    return grid, arr, curves, trades


def begins_inside_a_trade(lanes, trades):
    """Entries whose window begins with a position opened before it (and still open at from)."""
    return sum(any(e < int(L["from_bar"]) < x for e, x in tr) and int(L["from_bar"]) < int(L["to_bar"])
               for L, tr in zip(lanes, trades))


@functools.lru_cache(None)
def edge_reference(strategy, T):
    grid, lanes, curves, _ = edge_entries(strategy)
    return portfolio([(pos, eq, int(L["from_bar"]), int(L["to_bar"])) for (pos, eq), L in zip(curves, lanes)], T,
                     grid.annualization)


def curve_arrays(curves, stride):
    """The entries' curves as bt_replay returns them: (equity int64[n, stride], pos int8[n, stride],
    n_bars int32[n])."""
    eq = np.zeros((len(curves), stride), np.int64)
    ps = np.zeros((len(curves), stride), np.int8)
    nb = np.zeros(len(curves), np.int32)
    for i, (pos, e) in enumerate(curves):
        eq[i, :len(e)], ps[i, :len(pos)], nb[i] = e, pos, len(e)
    return eq, ps, nb


# ------------------------------------------------------------------------- the magnitude case
MAG_REPEAT = 48
MAG_IDS = (11, 12)
PMAX = 2**31 - 1


@functools.lru_cache(None)
def magnitude_case():
    """(grid, series [(h, l, c)], lanes, curves, reference at T = 300). Two 300-bar symbols near the
    2^31-tick ceiling: the golden near_max series (closes within 4,000 ticks of 2^31, moves of at
    most 3,926 ticks) and a doubling cycle 1, 2, .., 2^30, 2^31 - 1 that crashes back to 1 (the
    largest moves the oracle spec allows). Every SMA lane of both, MAG_REPEAT times each.

    The golden series alone cannot carry |pnl[t]| past 2^32: 2^20 entries, the most a call takes,
    times its largest move is 4.12e9 < 2^32. The cycle can: a bar's move is up to 2^31 - 2 ticks."""
    edge = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "edge.json")))
    near = next(x for x in edge if x["name"] == "near_max")
    cyc = np.asarray([1 << i for i in range(31)] + [PMAX], np.int64)[np.arange(300) % 32]
    series = [tuple(np.asarray(near[k], np.int32) for k in ("h", "l", "c")),
              tuple(np.ascontiguousarray(v, np.int32) for v in
                    (np.minimum(cyc + cyc // 8, PMAX), np.maximum(cyc - cyc // 8, 1), cyc))]
    grid = D.Grid.sma([1, 2, 3], [2, 7, 40])
    lanes = np.zeros(2 * grid.n_params * MAG_REPEAT, D.PF_LANE_DTYPE)
    curves = []
    for s, ohlc in enumerate(series):
        for p in range(grid.n_params):
            _, tr = oracle_lane("sma", grid, p, ohlc, cap=R.ORC_CAP)
            pos, eq = curves_from_trades(ohlc[2], tr)
            for _ in range(MAG_REPEAT):
                lanes[len(curves)] = (MAG_IDS[s], p, 0, WHOLE)
                curves.append((pos.tolist(), eq.tolist()))
    ref = portfolio([(pos, eq, 0, WHOLE) for pos, eq in curves], 300, grid.annualization)
    return grid, series, lanes, curves, ref
