"""Reference for the net-of-costs call (tests only), from the text of docs/costs_spec.md in plain
Python ints: one lane's record per fee level from a complete oracle trade list and the gross equity
curve of replay_ref.curves_from_trades, the per-(parameter, level) aggregate of a record array, and
the references of the shared cases (random_cases.lane_case, limit_cases family A, the ragged rows,
family A repeated to many rows), built once per process and not to be modified by a test. It shares
no code with csrc/costs.cpp.

Also here: the budget under which plan_costs takes a given number of rows per chunk (rows_budget),
restated from the text of plan.h; the CPU file holds it to the plan driver."""
import functools

import numpy as np

import dbx_amd as D
import limit_cases as LC
import random_cases as RC
import tradestats_ref as T
from replay_ref import curves_from_trades, oracle_lane

M64 = (1 << 64) - 1
# the ladder of the GPU tests: free, one tick a side, five basis points, a mixed level, the limit
LEVELS = ((0, 0), (1, 0), (0, 5), (7, 13), (2**20, 1000))
LIMIT = ((2**20, 1000),)


def fee(px, level):
    """fee_j(px) = fixed_j + floor(px * bps_j / 10000)."""
    fixed, bps = level
    return fixed + px * bps // 10000


def bar_fees(trades, level):
    """{bar: f_t} over the bars with a fill."""
    f = {}
    for e, x, _, epx, xpx in trades:
        f[e] = f.get(e, 0) + fee(epx, level)
        f[x] = f.get(x, 0) + fee(xpx, level)
    return f


def net_curve(trades, equity, level):
    """[N_t] of every bar: the gross equity less the fees of the fills up to and including t."""
    f = bar_fees(trades, level)
    out, paid = [], 0
    for t, E in enumerate(equity):
        paid += f.get(t, 0)
        out.append(E - paid)
    return out


def net_trades(trades, level):
    """[net_i] in closing order."""
    return [side * (xpx - epx) - fee(epx, level) - fee(xpx, level) for _, _, side, epx, xpx in trades]


def lane_costs(trades, equity, level):
    """Every field of bt_cost_rec as a dict of Python ints (s2 whole, not split). `trades`:
    tradestats_ref.trade_tuples; `equity`: the gross E_t of every bar."""
    E = [int(x) for x in equity]
    N = net_curve(trades, E, level)
    net = net_trades(trades, level)
    r = {"n_trades": len(trades), "n_win": sum(x > 0 for x in net), "n_loss": sum(x < 0 for x in net), "n_bars": len(E),
         "pnl": N[-1], "fees": sum(bar_fees(trades, level).values()),
         "turnover": sum(epx + xpx for _, _, _, epx, xpx in trades),
         "win_sum": sum(x for x in net if x > 0), "loss_sum": sum(-x for x in net if x < 0),
         "s2": sum((b - a) ** 2 for a, b in zip([0] + N[:-1], N))}
    peak, cur = [], 0
    for x in N:
        cur = max(cur, x)
        peak.append(cur)
    dd = [p - x for p, x in zip(peak, N)]
    r["mdd"] = max(dd)
    r["mdd_bar"] = dd.index(r["mdd"]) if r["mdd"] > 0 else -1      # the smallest t with dd_t = mdd
    r["underwater_bars"] = sum(x < p for x, p in zip(N, peak))
    return r


def as_record(r):
    out = np.zeros(1, D.COST_DTYPE)
    for f in D.COST_DTYPE.names:
        if f == "s2_lo":
            out[f] = r["s2"] & M64
        elif f == "s2_hi":
            out[f] = r["s2"] >> 64
        else:
            out[f] = r[f]
    return out[0]


def lane_records(close, trades, levels):
    """COST_DTYPE[C] of one lane from its symbol's closes and its complete oracle trade list."""
    _, eq = curves_from_trades(close, trades)
    tr, eq = T.trade_tuples(trades), eq.tolist()
    return np.array([as_record(lane_costs(tr, eq, lv)) for lv in levels], D.COST_DTYPE)


def s2_of(rec):
    return (int(rec["s2_hi"]) << 64) | int(rec["s2_lo"])


def aggregate(recs):
    """COST_AGG_DTYPE[P, C] from an S x P x C record array, in Python ints."""
    S, P, C = recs.shape
    out = np.zeros((P, C), D.COST_AGG_DTYPE)
    for p in range(P):
        for j in range(C):
            col, a = recs[:, p, j], out[p, j]
            a["n_sym"] = S
            a["n_traded"] = sum(int(x) > 0 for x in col["n_trades"])
            a["n_profit"] = sum(int(x) > 0 for x in col["pnl"])
            a["trades"] = sum(int(x) for x in col["n_trades"])
            a["pnl"] = sum(int(x) for x in col["pnl"])
            a["fees"] = sum(int(x) for x in col["fees"])
            a["mdd_max"] = max((int(x) for x in col["mdd"]), default=0)
    return out


assert_same = T.assert_same


# ------------------------------------------------------------------------------ shared references
@functools.lru_cache(None)
def random_refs(strategy, seed, levels=LEVELS):
    """(recs S x P x C, agg P x C) of random_cases.lane_case(strategy, seed), read-only."""
    c, r = RC.lane_case(strategy, seed), RC.lane_refs(strategy, seed)
    S, P = len(c.series), c.grid.n_params
    recs = np.zeros((S, P, len(levels)), D.COST_DTYPE)
    for s in range(S):
        for p in range(P):
            tr, eq = T.trade_tuples(r.lanes[s][p][1]), r.curves[s][p][1].tolist()
            for j, lv in enumerate(levels):
                recs[s, p, j] = as_record(lane_costs(tr, eq, lv))
    agg = aggregate(recs)
    recs.setflags(write=False)
    agg.setflags(write=False)
    return recs, agg


@functools.lru_cache(None)
def family_a_refs(name, levels=LIMIT):
    """(grid, series [(c, h, l)], recs S x P x C) of limit_cases family A, the doubling cycles."""
    strategy, grid, series, rows = LC._a_case(name)
    recs = np.zeros((len(series), grid.n_params, len(levels)), D.COST_DTYPE)
    for s, ((c, _, _), (summ, trades)) in enumerate(zip(series, rows)):
        for p in range(grid.n_params):
            assert int(summ[p]["n_trades"]) == len(trades[p]) <= LC.CAP_A, "family A keeps complete trade lists"
            recs[s, p] = lane_records(c, trades[p], levels)
    recs.setflags(write=False)
    return grid, series, recs


@functools.lru_cache(None)
def family_a_many_rows(name, levels=LIMIT):
    """(grid, series * A_ROWS, recs A_ROWS x P x C): row r is series r mod S of family A."""
    grid, series, recs = family_a_refs(name, levels)
    rows = np.arange(T.A_ROWS) % len(series)
    many = recs[rows]
    many.setflags(write=False)
    return grid, [series[r] for r in rows], many


def case_lanes(strategy, grid, series):
    """[[(trade tuples, equity list)]] of a small crafted case: `series` as [(h, l, c)]."""
    out = []
    for ohlc in series:
        row = []
        for p in range(grid.n_params):
            summ, tr = oracle_lane(strategy, grid, p, ohlc, cap=len(ohlc[2]))
            assert int(summ["n_trades"]) == (0 if tr is None else len(tr))
            row.append((T.trade_tuples(tr), curves_from_trades(ohlc[2], tr)[1].tolist()))
        out.append(row)
    return out


def case_series(strategy, grid, series, levels=LEVELS, lanes=None):
    """The reference records S x P x C of a small crafted case: `series` as [(h, l, c)]."""
    lanes = lanes or case_lanes(strategy, grid, series)
    recs = np.zeros((len(series), grid.n_params, len(levels)), D.COST_DTYPE)
    for s, row in enumerate(lanes):
        for p, (tr, eq) in enumerate(row):
            for j, lv in enumerate(levels):
                recs[s, p, j] = as_record(lane_costs(tr, eq, lv))
    return recs


def rows_budget(P, C, rows):
    """The staging budget under which plan_costs takes exactly `rows` dataset rows per chunk
    (all-lanes mode): agg[P * C] rounded up to 256 bytes, one rounding of the records, `rows` rows."""
    return (P * C * D.COST_AGG_DTYPE.itemsize + 255) // 256 * 256 + 256 + rows * P * C * D.COST_DTYPE.itemsize
