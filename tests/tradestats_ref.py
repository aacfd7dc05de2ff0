"""Reference for the trade statistics (tests only), from the text of docs/tradestats_spec.md in
plain Python ints: one lane's record from a complete oracle trade list (closing order) and the
equity curve of replay_ref.curves_from_trades, the per-parameter aggregate of a record matrix, and
the references of the shared cases (random_cases.lane_case, limit_cases family A, the ragged rows,
family A repeated to many rows, the wide grids), built once per process and not to be modified by a
test. lane_stats_fast is the same record from numpy arrays, for rows too long for a Python loop;
tests/test_tradestats_cpu.py pins it to lane_stats field for field.

Also here: the arithmetic of tstats_agg_kernel's slices (agg_slice_rows) and the budget under which
plan_tstats takes a given number of rows per chunk (rows_budget), restated from the text of plan.h
and k_tstats.hip; the CPU file holds both to the plan driver."""
import functools

import numpy as np

import dbx_amd as D
import limit_cases as LC
import random_cases as RC
from replay_ref import curves_from_trades

M64 = (1 << 64) - 1
SUM_FIELDS = ("n_trades", "n_win", "n_loss", "n_long", "n_long_win", "hold_sum", "hold_win", "gross_win", "gross_loss")
MAX_FIELDS = (("max_win_streak", "max_win_streak"), ("max_loss_streak", "max_loss_streak"), ("hold_max", "hold_max"),
              ("max_underwater", "max_underwater"), ("max_win", "max_win"), ("max_loss", "max_loss"), ("mdd_max", "mdd"))


def _mix(entry_bar, exit_bar, side):
    """docs/oracle_spec.md §4: one mixed 64-bit word per trade."""
    w = entry_bar | exit_bar << 31 | (1 if side > 0 else 0) << 62
    z = ((w ^ (w >> 29)) * 0xBF58476D1CE4E5B9) & M64
    return z ^ (z >> 32)


def trade_tuples(trades):
    """[(entry_bar, exit_bar, side, entry_px, exit_px)] in Python ints."""
    if trades is None or len(trades) == 0:
        return []
    return list(zip(*(trades[f].tolist() for f in ("entry_bar", "exit_bar", "side", "entry_px", "exit_px"))))


def longest_run(flags):
    best = run = 0
    for f in flags:
        run = run + 1 if f else 0
        best = max(best, run)
    return best


def lane_stats(trades, equity):
    """Every field of bt_tstats as a dict of Python ints (sq whole, not split). `trades`:
    trade_tuples in closing order; `equity`: E_t of every bar."""
    E = [int(x) for x in equity]
    B = len(E)
    pnl = [side * (xpx - epx) for _, _, side, epx, xpx in trades]
    hold = [x - e for e, x, _, _, _ in trades]
    sides = [side for _, _, side, _, _ in trades]
    win = [p > 0 for p in pnl]
    loss = [p < 0 for p in pnl]
    r = {"n_trades": len(trades), "n_win": sum(win), "n_loss": sum(loss), "status": 0,
         "n_long": sum(s > 0 for s in sides), "n_long_win": sum(s > 0 and w for s, w in zip(sides, win)),
         # a flat trade is neither: it ends a run of either kind
         "max_win_streak": longest_run(win), "max_loss_streak": longest_run(loss),
         "hold_sum": sum(hold), "hold_win": sum(h for h, w in zip(hold, win) if w), "hold_max": max(hold, default=0),
         "n_bars": B,
         "gross_win": sum(p for p in pnl if p > 0), "gross_loss": sum(-p for p in pnl if p < 0),
         "max_win": max([p for p in pnl if p > 0], default=0), "max_loss": max([-p for p in pnl if p < 0], default=0),
         "sq": sum(p * p for p in pnl),
         "hash": sum(_mix(e, x, s) for e, x, s, _, _ in trades) & M64}
    peak, cur = [], 0
    for x in E:
        cur = max(cur, x)
        peak.append(cur)
    dd = [p - x for p, x in zip(peak, E)]
    r["mdd"] = max(dd, default=0)
    if r["mdd"] > 0:
        r["mdd_bar"] = dd.index(r["mdd"])                     # the smallest t with dd_t = mdd
        r["peak_bar"] = E.index(peak[r["mdd_bar"]])           # the smallest t' with E_t' = that peak
        assert r["peak_bar"] <= r["mdd_bar"]
    else:
        r["mdd_bar"] = r["peak_bar"] = -1
    under = [x < p for x, p in zip(E, peak)]
    r["underwater_bars"] = sum(under)
    r["max_underwater"] = longest_run(under)
    return r


def as_record(r):
    """lane_stats' dict as one TSTATS_DTYPE record."""
    out = np.zeros(1, D.TSTATS_DTYPE)
    for f in D.TSTATS_DTYPE.names:
        if f == "sq_lo":
            out[f] = r["sq"] & M64
        elif f == "sq_hi":
            out[f] = r["sq"] >> 64
        else:
            out[f] = r[f]
    return out[0]


def lane_record(close, trades):
    """One lane's record from its symbol's closes and its complete oracle trade list."""
    _, eq = curves_from_trades(close, trades)
    return as_record(lane_stats(trade_tuples(trades), eq.tolist()))


def sq_of(rec):
    return (int(rec["sq_hi"]) << 64) | int(rec["sq_lo"])


def aggregate(recs):
    """TSTATS_AGG_DTYPE[P] from an S x P record matrix, in Python ints."""
    S, P = recs.shape
    out = np.zeros(P, D.TSTATS_AGG_DTYPE)
    for p in range(P):
        col = recs[:, p]
        a = out[p]
        a["n_sym"] = S
        a["n_traded"] = sum(int(x) > 0 for x in col["n_trades"])
        for f in SUM_FIELDS:
            a[f] = sum(int(x) for x in col[f])
        for f, src in MAX_FIELDS:
            a[f] = max((int(x) for x in col[src]), default=0)
        sq = sum(sq_of(x) for x in col)
        a["sq_lo"], a["sq_hi"] = sq & M64, sq >> 64
    return out


def assert_same(got, want, where):
    """Field by field, the first difference named."""
    assert got.dtype == want.dtype and got.shape == want.shape, f"{where}: {got.dtype} {got.shape} vs {want.shape}"
    for f in want.dtype.names:
        bad = np.argwhere(np.atleast_1d(got[f] != want[f]))
        if len(bad):
            i = tuple(int(x) for x in bad[0])
            g, w = np.atleast_1d(got[f])[i], np.atleast_1d(want[f])[i]
            raise AssertionError(f"{where}: {f}{list(i)} = {g}, want {w} ({len(bad)} records differ)")
    assert got.tobytes() == want.tobytes(), where


# ------------------------------------------------------------------------------ shared references
@functools.lru_cache(None)
def random_refs(strategy, seed):
    """(recs S x P, agg P) of random_cases.lane_case(strategy, seed), read-only."""
    c, r = RC.lane_case(strategy, seed), RC.lane_refs(strategy, seed)
    S, P = len(c.series), c.grid.n_params
    recs = np.zeros((S, P), D.TSTATS_DTYPE)
    for s in range(S):
        for p in range(P):
            recs[s, p] = as_record(lane_stats(trade_tuples(r.lanes[s][p][1]), r.curves[s][p][1].tolist()))
    agg = aggregate(recs)
    recs.setflags(write=False)
    agg.setflags(write=False)
    return recs, agg


@functools.lru_cache(None)
def family_a_refs(name):
    """(grid, series [(c, h, l)], recs S x P) of limit_cases family A, the doubling cycles."""
    strategy, grid, series, rows = LC._a_case(name)
    recs = np.zeros((len(series), grid.n_params), D.TSTATS_DTYPE)
    for s, ((c, _, _), (summ, trades)) in enumerate(zip(series, rows)):
        for p in range(grid.n_params):
            assert int(summ[p]["n_trades"]) == len(trades[p]) <= LC.CAP_A, "family A keeps complete trade lists"
            recs[s, p] = lane_record(c, trades[p])
    recs.setflags(write=False)
    return grid, series, recs


def case_series(strategy, grid, series):
    """The oracle's complete trade lists and reference records of a small crafted case: `series`
    as [(h, l, c)]; returns recs S x P."""
    from replay_ref import oracle_lane
    recs = np.zeros((len(series), grid.n_params), D.TSTATS_DTYPE)
    for s, ohlc in enumerate(series):
        for p in range(grid.n_params):
            summ, tr = oracle_lane(strategy, grid, p, ohlc, cap=len(ohlc[2]))
            assert int(summ["n_trades"]) == (0 if tr is None else len(tr))
            recs[s, p] = lane_record(ohlc[2], tr)
    return recs


# ------------------------------------------------------------------- the vectorised reference
def longest_run_fast(flags):
    """longest_run by differences of the positions where a run begins and ends."""
    edge = np.diff(np.concatenate([[0], np.asarray(flags, np.int8), [0]]))
    begin, end = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)
    return int((end - begin).max()) if len(begin) else 0


def lane_stats_fast(trades, equity):
    """lane_stats from the oracle's trade array (or None) and the equity array, in numpy: the trade
    fields in int64 (|pnl| < 2^31 and at most 2^22 trades: no sum leaves int64) with sq summed in
    Python ints, the drawdown fields from np.maximum.accumulate, the run lengths by
    longest_run_fast."""
    E = np.asarray(equity, np.int64)
    n = 0 if trades is None else len(trades)
    col = lambda f: trades[f].astype(np.int64) if n else np.zeros(0, np.int64)
    ebar, xbar, side = col("entry_bar"), col("exit_bar"), col("side")
    pnl = side * (col("exit_px") - col("entry_px"))
    hold = xbar - ebar
    win, loss, lng = pnl > 0, pnl < 0, side > 0
    w = (ebar | xbar << 31 | lng.astype(np.int64) << 62).astype(np.uint64)
    z = (w ^ (w >> np.uint64(29))) * np.uint64(0xBF58476D1CE4E5B9)          # uint64: mod 2^64
    r = {"n_trades": n, "n_win": int(win.sum()), "n_loss": int(loss.sum()), "status": 0,
         "n_long": int(lng.sum()), "n_long_win": int((lng & win).sum()),
         "max_win_streak": longest_run_fast(win), "max_loss_streak": longest_run_fast(loss),
         "hold_sum": int(hold.sum()), "hold_win": int(hold[win].sum()), "hold_max": int(hold.max()) if n else 0,
         "n_bars": len(E),
         "gross_win": int(pnl[win].sum()), "gross_loss": int(-pnl[loss].sum()),
         "max_win": int(pnl[win].max()) if win.any() else 0, "max_loss": int(-pnl[loss].min()) if loss.any() else 0,
         "sq": sum(x * x for x in pnl.tolist()),
         "hash": int((z ^ (z >> np.uint64(32))).sum(dtype=np.uint64)) if n else 0}
    peak = np.maximum.accumulate(np.maximum(E, 0))
    dd = peak - E
    r["mdd"] = int(dd.max()) if len(E) else 0
    if r["mdd"] > 0:
        r["mdd_bar"] = int(np.argmax(dd))                                   # the first of the maxima
        r["peak_bar"] = int(np.argmax(E == peak[r["mdd_bar"]]))             # the first bar at that peak
    else:
        r["mdd_bar"] = r["peak_bar"] = -1
    under = E < peak
    r["underwater_bars"] = int(under.sum())
    r["max_underwater"] = longest_run_fast(under)
    return r


# ------------------------------------------------------ the reduction's geometry (k_tstats.hip)
def rows_budget(P, rows):
    """The staging budget under which plan_tstats takes exactly `rows` dataset rows per chunk
    (all-lanes mode): agg[P] rounded up to 256 bytes, one rounding of the records, `rows` rows."""
    return (P * D.TSTATS_AGG_DTYPE.itemsize + 255) // 256 * 256 + 256 + rows * P * D.TSTATS_DTYPE.itemsize


def agg_slice_rows(n_rows, slices):
    """[(r0, r1)] of tstats_agg_kernel's grid y over a chunk of n_rows rows: per = ceil(n_rows /
    slices) rows each; a slice with r0 >= r1 is empty and returns at once."""
    per = -(-n_rows // slices)
    return [(y * per, min(y * per + per, n_rows)) for y in range(slices)]


def slice_low_words(recs, p, chunks, slices):
    """What each non-empty slice of each chunk adds into agg[p].sq_lo: its rows' sum of squares
    mod 2^64. `chunks`: [(r0, r1)] dataset rows."""
    out = []
    for c0, c1 in chunks:
        for r0, r1 in agg_slice_rows(c1 - c0, slices):
            if r0 < r1:
                out.append(sum(sq_of(x) for x in recs[c0 + r0:c0 + r1, p]) & M64)
    return out


A_ROWS = 205          # family A's series repeated cyclically: 4 slices at the default budget
A_CHUNK_ROWS = (100, 200)   # rows per chunk under the two budgets of the many-row tests


@functools.lru_cache(None)
def family_a_many_rows(name):
    """(grid, series [(c, h, l)] * A_ROWS, recs A_ROWS x P): row r is series r mod S of family A,
    and its reference records repeat with it."""
    grid, series, recs = family_a_refs(name)
    rows = np.arange(A_ROWS) % len(series)
    many = recs[rows]
    many.setflags(write=False)
    return grid, [series[r] for r in rows], many


RAGGED = (1, 2, 64, 65, 130, 700)
RAGGED_GRIDS = {"sma": lambda: D.Grid.sma([1, 3, 10], [2, 20]),
                "ema_ols": lambda: D.Grid.ema_ols([3, 20], [4, 30], band_bps=5),
                "boll": lambda: D.Grid.boll([5, 20], [2, 3], [30], [60, 400], k_den=2)}


def ragged_series(strategy, lengths=RAGGED, kinds=RC.KINDS):
    """[(h, l, c)] of the given lengths, one path kind after the other (seeded by strategy)."""
    rng = np.random.default_rng([0x7A66, RC.STRATEGIES.index(strategy)])
    series = []
    for i, n in enumerate(lengths):
        c = RC._series(rng, n, kinds[i % len(kinds)] if n > 2 else "walk")
        h, lo = RC._ohlc(rng, c)
        series.append((h, lo, c))
    return series


# two SMA grids wider than one 64-thread block of the reduction: 100 parameters (one block of 128
# threads) and 272 = 4 * 64 + 16 (two blocks of 256, the second with 240 threads past P)
WIDE_GRIDS = {"p100": lambda: D.Grid.sma(list(range(1, 11)), list(range(12, 52, 4))),
              "p272": lambda: D.Grid.sma(list(range(1, 18)), list(range(18, 66, 3)))}
WIDE_ROWS = (65, 130, 300)


@functools.lru_cache(None)
def wide_grid_refs(name):
    """(grid, series [(h, l, c)], recs 3 x P) of a wide grid on three short ragged rows."""
    grid = WIDE_GRIDS[name]()
    series = ragged_series("sma", WIDE_ROWS, ("walk", "spiky"))
    recs = case_series("sma", grid, series)
    recs.setflags(write=False)
    return grid, series, recs
