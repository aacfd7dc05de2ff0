"""Reference for the tail-risk call (tests only), from the text of docs/tail_spec.md in plain Python
ints: one lane's record and its per-level order statistics from the position and equity curves
that random_cases.lane_refs already holds (d = diff(equity, prepend 0), held from pos[t - 1], a plain
sorted), the references of the shared cases (random cases, ragged rows, limit family A), built once
per process and not to be modified by a test, the restatement of TailRisk's derived views, and the
budget under which plan_tail takes a given number of units per chunk (rows_budget), restated from
the text of plan.h. It shares no code with csrc/tail.cpp."""
import bisect
import functools
import math
from statistics import NormalDist

import numpy as np

import dbx_amd as D
import limit_cases as LC
import random_cases as RC
import tradestats_ref as T
from replay_ref import curves_from_trades, oracle_lane

M64 = (1 << 64) - 1
# the level set of the issue: the ends of the range, a repeat, and 999,999 ppm beside 10^6
LEVELS = (1, 10_000, 50_000, 250_000, 500_000, 1_000_000, 50_000, 999_999)
WHOLE = None


def counted(pos, equity, window=WHOLE, held=False):
    """[(t, d_t)] of the counted bars of one lane; `window`: (from, to) or None for the whole row."""
    E = [int(x) for x in equity]
    B = len(E)
    frm, to = (0, B) if window is None or tuple(window) == (0, 0) else window
    out = []
    for t in range(frm, min(to, B)):
        if held and not (t >= 1 and int(pos[t - 1]) != 0):
            continue
        out.append((t, E[t] - (E[t - 1] if t else 0)))
    return out, max(min(to, B) - frm, 0)


def row_tail(bars, n_window, levels=LEVELS):
    """(record dict, [quantile dict]) of the counted (t, d) of one lane."""
    ds = [d for _, d in bars]
    n = len(ds)
    r = {"n": n, "n_window": n_window, "n_pos": sum(d > 0 for d in ds), "n_neg": sum(d < 0 for d in ds),
         "min_d": min(ds, default=0), "max_d": max(ds, default=0), "s1": sum(ds), "s1_neg": sum(d for d in ds if d < 0),
         "s2": sum(d * d for d in ds), "s2_neg": sum(d * d for d in ds if d < 0), "s3": sum(d ** 3 for d in ds),
         "s4": sum(d ** 4 for d in ds)}
    r["min_bar"] = next((t for t, d in bars if d == r["min_d"]), -1)
    r["max_bar"] = next((t for t, d in bars if d == r["max_d"]), -1)
    srt = sorted(ds)
    qs = []
    for a in levels:
        if n == 0:
            qs.append({"var": 0, "es_sum": 0, "k": 0, "n_lt": 0})
            continue
        k = -(-n * a // 1_000_000)
        assert 1 <= k <= n
        qs.append({"var": srt[k - 1], "es_sum": sum(srt[:k]), "k": k, "n_lt": bisect.bisect_left(srt, srt[k - 1])})
    return r, qs


def as_records(r, qs):
    rec = np.zeros((), D.TAIL_DTYPE)
    for f in ("n", "n_window", "n_pos", "n_neg", "min_bar", "max_bar", "min_d", "max_d", "s1", "s1_neg"):
        rec[f] = r[f]
    for f in ("s2", "s2_neg", "s3"):
        rec[f + "_lo"], rec[f + "_hi"] = r[f] & M64, r[f] >> 64
    rec["s4"] = [(r["s4"] >> (64 * i)) & M64 for i in range(3)]
    assert r["s4"] < 1 << 192
    q = np.zeros(len(qs), D.TAIL_Q_DTYPE)
    for j, x in enumerate(qs):
        q[j] = (x["var"], x["es_sum"], x["k"], x["n_lt"])
    return rec, q


def lanes_tail(curves, window=WHOLE, held=False, levels=LEVELS):
    """(TAIL_DTYPE[n], TAIL_Q_DTYPE[n, Q]) of [(pos, equity)]."""
    recs, qs = np.zeros(len(curves), D.TAIL_DTYPE), np.zeros((len(curves), len(levels)), D.TAIL_Q_DTYPE)
    for i, (pos, eq) in enumerate(curves):
        recs[i], qs[i] = as_records(*row_tail(*counted(pos, eq, window, held), levels))
    return recs, qs


def rows_tail(d, levels=LEVELS):
    """The reference of tail_of: every entry of every row of d counts, bars are row indices."""
    d = np.asarray(d)
    recs, qs = np.zeros(len(d), D.TAIL_DTYPE), np.zeros((len(d), len(levels)), D.TAIL_Q_DTYPE)
    for i, row in enumerate(d.tolist()):
        recs[i], qs[i] = as_records(*row_tail(list(enumerate(row)), len(row), levels))
    return recs, qs


def wide(rec, f):
    return (int(rec[f + "_hi"]) << 64) | int(rec[f + "_lo"])


def s4_of(rec):
    return sum(int(x) << (64 * i) for i, x in enumerate(rec["s4"].tolist()))


def assert_same(got, want, where):
    """Field by field, the first difference named."""
    assert got.dtype == want.dtype and got.shape == want.shape, f"{where}: {got.dtype} {got.shape} vs {want.shape}"
    for f in want.dtype.names:
        g, w = got[f], want[f]
        bad = np.argwhere(np.atleast_1d(g != w))
        if len(bad):
            i = tuple(int(x) for x in bad[0])
            raise AssertionError(f"{where}: {f}{list(i)} = {np.atleast_1d(g)[i]}, want {np.atleast_1d(w)[i]} "
                                 f"({len(bad)} values differ)")
    assert got.tobytes() == want.tobytes(), where


# ------------------------------------------------------------------------------ shared references
def cut_window(bars):
    """One window that begins inside every row but the shortest ones and ends inside the longest:
    rows end before it, inside it and after its start."""
    lo, hi = min(bars), max(bars)
    return (max(lo // 3, 1), max(hi - hi // 4, max(lo // 3, 1) + 1))


@functools.lru_cache(None)
def random_refs(strategy, seed, held=False, cut=False):
    """(recs S x P, quantiles S x P x Q, window) of random_cases.lane_case(strategy, seed), read-only."""
    c, r = RC.lane_case(strategy, seed), RC.lane_refs(strategy, seed)
    S, P = len(c.series), c.grid.n_params
    window = cut_window(c.bars) if cut else WHOLE
    recs, qs = lanes_tail([r.curves[s][p] for s in range(S) for p in range(P)], window, held)
    recs, qs = recs.reshape(S, P), qs.reshape(S, P, len(LEVELS))
    recs.setflags(write=False)
    qs.setflags(write=False)
    return recs, qs, window


def list_refs(c, recs, qs):
    """The rows of an S x P reference in the order of the case's replay_lanes."""
    row = {i: s for s, i in enumerate(c.ids)}
    idx = [(row[i], p) for i, p in c.replay_lanes]
    return (np.array([recs[s, p] for s, p in idx], D.TAIL_DTYPE),
            np.array([qs[s, p] for s, p in idx], D.TAIL_Q_DTYPE))


@functools.lru_cache(None)
def family_a_curves(name):
    """(grid, series [(c, h, l)], [(pos, equity)] row-major) of limit_cases family A."""
    strategy, grid, series, rows = LC._a_case(name)
    curves = []
    for (c, _, _), (summ, trades) in zip(series, rows):
        for p in range(grid.n_params):
            assert int(summ[p]["n_trades"]) == len(trades[p]) <= LC.CAP_A, "family A keeps complete trade lists"
            curves.append(curves_from_trades(c, trades[p]))
    return grid, series, curves


@functools.lru_cache(None)
def ragged_curves(strategy):
    """(grid, series [(h, l, c)], [(pos, equity)] row-major) of tradestats_ref's ragged rows."""
    series, grid = T.ragged_series(strategy), T.RAGGED_GRIDS[strategy]()
    curves = []
    for ohlc in series:
        for p in range(grid.n_params):
            summ, tr = oracle_lane(strategy, grid, p, ohlc, cap=len(ohlc[2]))
            assert int(summ["n_trades"]) == (0 if tr is None else len(tr))
            curves.append(curves_from_trades(ohlc[2], tr))
    return grid, series, curves


def as_curve_arrays(curves):
    """(equity int64[n, stride], pos int8[n, stride], n_bars int32[n]) as bt_replay returns them."""
    stride = max(len(eq) for _, eq in curves)
    eq, ps = np.zeros((len(curves), stride), np.int64), np.zeros((len(curves), stride), np.int8)
    for i, (p, e) in enumerate(curves):
        eq[i, :len(e)], ps[i, :len(p)] = e, p
    return eq, ps, np.array([len(e) for _, e in curves], np.int32)


# ------------------------------------------------------------------------------- derived views
def central(rec):
    n, s1, s2, s3, s4 = int(rec["n"]), int(rec["s1"]), wide(rec, "s2"), wide(rec, "s3"), s4_of(rec)
    return (n, s1, n * s2 - s1 ** 2, n ** 2 * s3 - 3 * n * s1 * s2 + 2 * s1 ** 3,
            n ** 3 * s4 - 4 * n ** 2 * s1 * s3 + 6 * n * s1 ** 2 * s2 - 3 * s1 ** 4)


def sgn(x):
    return (x > 0) - (x < 0)


def views(rec, ann=1):
    """{name: value} of one record's derived views, in the order of operations of the spec's §6."""
    n, s1, M2, M3, M4 = central(rec)
    neg, s2n = int(rec["s1_neg"]), wide(rec, "s2_neg")
    root = math.sqrt(float(ann))
    return {"mean": s1 / n if n else 0.0, "std": math.sqrt(M2) / n if n else 0.0,
            "skew": sgn(M3) * math.sqrt(M3 * M3 / M2 ** 3) if M2 else 0.0, "kurtosis": M4 / M2 ** 2 if M2 else 0.0,
            "sharpe": sgn(s1) * math.sqrt(s1 * s1 / M2) * root if M2 else 0.0,
            "sortino": sgn(s1) * math.sqrt(s1 * s1 / (n * s2n)) * root if n * s2n else 0.0,
            "gain_to_pain": s1 / -neg if neg else 0.0}


def phi(x):
    return 0.5 * (1.0 + math.erf(x / math.sqrt(2.0)))


def psr(rec, sr0=0.0):
    v = views(rec)
    n, sr = int(rec["n"]), v["sharpe"]
    den = 1.0 - v["skew"] * sr + (v["kurtosis"] - 1.0) / 4.0 * sr * sr
    return phi((sr - sr0) * math.sqrt(n - 1) / math.sqrt(den)) if n >= 2 and central(rec)[2] > 0 and den > 0 else 0.0


def dsr_threshold(V, N):
    g, Z = 0.5772156649015329, NormalDist().inv_cdf
    return math.sqrt(V) * ((1.0 - g) * Z(1.0 - 1.0 / N) + g * Z(1.0 - 1.0 / (N * math.e)))


# ------------------------------------------------------------------------------------ planner
def rows_budget(P, Q, pitch_words, units, list_mode=False):
    """The staging budget under which plan_tail takes exactly `units` units per chunk: the levels
    rounded up to 256 bytes, one rounding for each of the chunk's four regions, and per unit P lanes
    (1 in list mode, with a 16-byte request) of one record, Q quantile records and a row of
    pitch_words words (0 when the row lives in LDS)."""
    lane = 128 + Q * 24 + pitch_words * 4
    return (Q * 4 + 255) // 256 * 256 + 4 * 256 + units * ((16 + lane) if list_mode else P * lane)
