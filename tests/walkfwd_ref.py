"""Reference for the walk-forward tests (tests only), written from docs/walkforward_spec.md.

Fold records come from the C oracle's complete trade list of a lane: replay_ref.curves_from_trades
rebuilds pos_t and E_t, oracle_np.fixed_returns gives q_t and q2_t, and every sum is a Python int;
the Sharpe is the oracle's formula (oracle_np._sharpe). Steps and totals are plain loops over those
records. test_walkfwd_cpu.py pins the records to the oracle's whole-series summary and sums.

The two cases the CPU and the GPU tests share are built once per process (edge_case,
selection_case) and must not be modified by a test."""
import functools
import struct

import numpy as np

import dbx_amd as D
import oracle_np as N
from replay_ref import curves_from_trades, gen_hlc, oracle_lane

ORC_CAP = 1 << 15   # the oracle's trade lists are complete
MASK = (1 << 64) - 1


def _split(v):
    """Python int -> (lo, hi) words of an int128."""
    return v & MASK, v >> 64


def _join(lo, hi):
    return (int(hi) << 64) | int(lo)


def key(x):
    """The engine's orderable Sharpe (oracle spec §5)."""
    u = struct.unpack("<Q", struct.pack("<d", float(x)))[0]
    return (~u & MASK) if u >> 63 else (u | 1 << 63)


def n_ret(first_bar, n_bars):
    """Return bars of a fold: its bars but bar 0."""
    return n_bars - (1 if first_bar == 0 and n_bars > 0 else 0)


def lane_folds(c, trades, bounds, ann, out):
    """out[k] (FOLD_DTYPE) for the K folds of one lane with closes c and complete trade list."""
    B = len(c)
    pos, eq = curves_from_trades(c, trades)
    pos, eq = pos.tolist(), eq.tolist()
    q, q2 = fixed_q(c)
    exits = [] if trades is None else [int(t["exit_bar"]) for t in trades]
    E = lambda b: eq[b - 1] if b > 0 else 0
    for k in range(len(bounds) - 1):
        ck, ck1 = min(bounds[k], B), min(bounds[k + 1], B)
        rec = out[k]
        rec["first_bar"] = ck
        if ck1 <= ck:
            continue
        s1 = s2 = expo = 0
        for t in range(max(ck, 1), ck1):
            if pos[t - 1]:
                s1 += pos[t - 1] * q[t]
                s2 += q2[t]
                expo += 1
        base = E(ck)
        peak = mdd = 0
        for t in range(ck, ck1):
            d = eq[t] - base
            peak = max(peak, d)
            mdd = max(mdd, peak - d)
        rec["n_bars"] = ck1 - ck
        rec["n_trades"] = sum(ck <= x < ck1 for x in exits)
        rec["pnl"] = E(ck1) - base
        rec["mdd"] = mdd
        rec["exposure"] = expo
        rec["sharpe"] = N._sharpe(s1, s2, n_ret(ck, ck1 - ck) + 1, ann)
        (rec["s1_lo"], rec["s1_hi"]), (rec["s2_lo"], rec["s2_hi"]) = _split(s1), _split(s2)


_Q = {}


def fixed_q(c):
    """oracle_np.fixed_returns, once per series."""
    k = (len(c), hash(np.asarray(c).tobytes()))
    if k not in _Q:
        if len(_Q) > 64:
            _Q.clear()
        _Q[k] = N.fixed_returns(c)
    return _Q[k]


def ref_folds(strategy, grid, series, bounds):
    """(folds FOLD_DTYPE[S, P, K], lanes): every lane's fold records; lanes[s][p] = (oracle
    summary, trade list) for the tests that look at the trades."""
    S, P, K = len(series), grid.n_params, len(bounds) - 1
    folds = np.zeros((S, P, K), D.FOLD_DTYPE)
    lanes = []
    for s, ohlc in enumerate(series):
        row = []
        for p in range(P):
            summ, tr = oracle_lane(strategy, grid, p, ohlc, cap=ORC_CAP)
            assert int(summ["n_trades"]) <= ORC_CAP
            lane_folds(ohlc[2], tr, bounds, grid.annualization, folds[s, p])
            row.append((summ, tr))
        lanes.append(row)
    return folds, lanes


def ref_steps(folds, ids, train, ann):
    """(steps WF_STEP_DTYPE[S, n_steps], total FOLD_DTYPE[S], tied) by the spec's loops; tied[s][i]
    is how many lanes share step i's best training Sharpe (0 for a step without a pick)."""
    S, P, K = folds.shape
    j0 = max(train, 1)
    steps = np.zeros((S, K - j0), D.WF_STEP_DTYPE)
    total = np.zeros(S, D.FOLD_DTYPE)
    tied = []
    for s in range(S):
        f = folds[s]
        nret = [n_ret(int(f[0, k]["first_bar"]), int(f[0, k]["n_bars"])) for k in range(K)]
        s1 = [[_join(f[p, k]["s1_lo"], f[p, k]["s1_hi"]) for k in range(K)] for p in range(P)]
        s2 = [[_join(f[p, k]["s2_lo"], f[p, k]["s2_hi"]) for k in range(K)] for p in range(P)]
        tied.append([])
        t1 = t2 = tn = 0
        first = True
        for j in range(j0, K):
            st = steps[s, j - j0]
            st["sym"], st["fold"], st["param"] = ids[s], j, -1
            st["oos"]["first_bar"] = f[0, j]["first_bar"]
            a = 0 if train == 0 else j - train
            n = sum(nret[a:j])
            if n == 0 or f[0, j]["n_bars"] == 0:
                tied[-1].append(0)
                continue
            sh = [N._sharpe(sum(s1[p][a:j]), sum(s2[p][a:j]), n + 1, ann) for p in range(P)]
            keys = [key(x) for x in sh]
            best = max(keys)
            bp = keys.index(best)               # ties to the lowest param
            tied[-1].append(keys.count(best))
            st["param"], st["train_sharpe"], st["oos"] = bp, sh[bp], f[bp, j]
            o = f[bp, j]
            if first:
                total[s]["first_bar"] = o["first_bar"]
                first = False
            for name in ("n_bars", "n_trades", "pnl", "exposure"):
                total[s][name] += o[name]
            total[s]["mdd"] = max(int(total[s]["mdd"]), int(o["mdd"]))
            t1 += s1[bp][j]
            t2 += s2[bp][j]
            tn += nret[j]
        (total[s]["s1_lo"], total[s]["s1_hi"]), (total[s]["s2_lo"], total[s]["s2_hi"]) = _split(t1), _split(t2)
        total[s]["sharpe"] = N._sharpe(t1, t2, tn + 1, ann)
    return steps, total, tied


def assert_same(got, want, what):
    """Structured arrays equal byte for byte (doubles by bits); the first difference is named."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {got.shape} vs {want.shape}"
    if got.tobytes() == want.tobytes():
        return
    g, w = got.reshape(-1), want.reshape(-1)
    for i in range(len(g)):
        if g[i].tobytes() != w[i].tobytes():
            idx = np.unravel_index(i, got.shape)
            raise AssertionError(f"{what}: record {tuple(int(x) for x in idx)} differs:\n got  {g[i]}\n want {w[i]}")


# ------------------------------------------------------------------------------ shared cases
EDGE_BARS = (1, 2, 3, 63, 64, 65, 128, 129, 1000)
EDGE_IDS = (907, 12, 500, 3, 77, 2_000_000, 41, 8, 650)
EDGE_BOUNDS = (0, 1, 2, 63, 64, 65, 128, 400, 999, 1000, 1200)
# windows below 64, between 64 and 1,000, and above 1,000 (longer than every series)
EDGE_GRIDS = {
    "sma": lambda: D.Grid.sma([3, 70, 1200], [5, 100, 300, 2000], annualization=98280),
    "ema_ols": lambda: D.Grid.ema_ols([5, 80, 1500], [4, 64, 200, 1100], band_bps=5),
    "boll": lambda: D.Grid.boll([5, 64, 150, 1200], [2, 3, 4], [30], [60], k_den=2),
}


@functools.lru_cache(None)
def edge_series():
    return [gen_hlc(0xED6E, i, b, 1) for i, b in zip(EDGE_IDS, EDGE_BARS)]


@functools.lru_cache(None)
def edge_case(strategy):
    """(grid, folds, lanes) of the edge set for one strategy."""
    grid = EDGE_GRIDS[strategy]()
    folds, lanes = ref_folds(strategy, grid, edge_series(), EDGE_BOUNDS)
    return grid, folds, lanes


def edge_counts(strategy):
    """Fold cells of the edge case (traded, open across the fold's end, exit on the fold's last
    bar other than the forced one at the series' end, entry on the fold's first bar), from the
    oracle's trade lists alone."""
    grid, folds, lanes = edge_case(strategy)
    traded = open_end = exit_last = entry_first = 0
    for s, B in enumerate(EDGE_BARS):
        for p in range(grid.n_params):
            tr = lanes[s][p][1]
            tr = [] if tr is None else [(int(t["entry_bar"]), int(t["exit_bar"])) for t in tr]
            for k in range(len(EDGE_BOUNDS) - 1):
                ck, ck1 = min(EDGE_BOUNDS[k], B), min(EDGE_BOUNDS[k + 1], B)
                if ck1 <= ck:
                    continue
                traded += any(ck <= x < ck1 for _, x in tr)
                open_end += any(e <= ck1 - 1 < x for e, x in tr)   # held after the fold's last bar
                exit_last += any(x == ck1 - 1 and x != B - 1 for _, x in tr)
                entry_first += any(e == ck for e, _ in tr)
    return traded, open_end, exit_last, entry_first


SEL_IDS = tuple(range(40, 46))
SEL_BARS = 600
SEL_SEED = 0x5E1
SEL_BOUNDS = tuple(range(0, 601, 100))


@functools.lru_cache(None)
def selection_series():
    return [gen_hlc(SEL_SEED, i, SEL_BARS, 0) for i in SEL_IDS]


@functools.lru_cache(None)
def selection_case():
    """(grid, folds, lanes) of the selection shape: the config-2 grid on 6 daily symbols."""
    grid = D.config2_grid()
    folds, lanes = ref_folds("sma", grid, selection_series(), SEL_BOUNDS)
    return grid, folds, lanes


@functools.lru_cache(None)
def selection_steps(train):
    grid, folds, _ = selection_case()
    return ref_steps(folds, SEL_IDS, train, grid.annualization)
