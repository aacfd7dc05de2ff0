"""Reference for the drawdown bootstrap (tests only), from the text of docs/drawdown_spec.md: the
resample plan of bootstrap_ref (drawn bar by bar: block start, then +1 mod T), every resampled path
walked bar by bar (the running sum, its peak from 0, the largest distance below it) and the records
that follow, the quantiles from sorted(). It forms no prefix row, no block summary and composes
nothing, so it shares nothing with k_ddboot.hip, and it is not ddboot.cpp.

The walks go through numpy int64 when max|d| * T < 2^62 (no partial sum can leave int64, so the
result is the Python-int one; test_ddboot_cpu.py pins the two to each other) and through Python ints
otherwise.

Also here: the shared cases of the two test files, built once per process and not to be modified by
a test, and anatomy(), which says from the reference alone which shapes a case reaches."""
import functools
from types import SimpleNamespace

import numpy as np

import dbx_amd as D
import bootstrap_ref as BR
import random_cases as RC

BIG = 2**31 - 1
LEVELS = (1, 500_000, 950_000, 1_000_000)
LIMITS = (0, 1, 5_000, 2**52)


def mdd(xs):
    """MDD of a sequence of Python ints: X_0 = 0, peak_m = max(0, X_1 .. X_m), max of peak_m - X_m."""
    x = peak = worst = 0
    for v in xs:
        x += v
        peak = max(peak, x)
        worst = max(worst, peak - x)
    return worst


def rank(B, alpha_ppm):
    return -(-B * alpha_ppm // 1_000_000)


def resampled_mdd(d, plan, exact=False):
    """[lane][b] Python ints: MDD of the lane's increments taken at the bars of resample b."""
    n, T = len(d), len(d[0])
    top = max((abs(x) for row in d for x in row), default=0)
    if not exact and top * T < 2**62:
        m = np.array(d, np.int64).reshape(n, T)
        out = []
        for bars in plan:
            X = np.cumsum(m[:, np.array(bars, np.int64)], axis=1)
            peak = np.maximum.accumulate(np.maximum(X, 0), axis=1)
            out.append((peak - X).max(axis=1))
        return np.stack(out, axis=1).tolist()
    return [[mdd(map(row.__getitem__, bars)) for bars in plan] for row in d]


def wide(v):
    return v & ((1 << 64) - 1), v >> 64


def records(d, star, levels, limits):
    """The outputs from the increments and MDD*_(i,b): SimpleNamespace(lanes, quantiles, reach, raw)
    as the arrays the library returns."""
    n, B = len(d), len(star[0])
    lanes = np.zeros(n, D.DD_LANE_DTYPE)
    q = np.zeros((n, len(levels)), np.int64)
    reach = np.zeros((n, len(limits)), np.int64)
    for i in range(n):
        obs = mdd(d[i])
        (lo1, hi1), (lo2, hi2) = wide(sum(star[i])), wide(sum(x * x for x in star[i]))
        lanes[i] = (sum(d[i]), obs, sum(x >= obs for x in star[i]), min(star[i]), max(star[i]), lo1, hi1, lo2, hi2)
        ordered = sorted(star[i])
        q[i] = [ordered[rank(B, a) - 1] for a in levels]
        reach[i] = [sum(x >= lim for x in star[i]) for lim in limits]
    return SimpleNamespace(lanes=lanes, quantiles=q, reach=reach, raw=np.array(star, np.int64).reshape(n, B))


def drawdown_risk(d, B, L, seed, levels=LEVELS, limits=LIMITS, exact=False):
    """The whole reference on increments d[n][T] (lists of Python ints)."""
    d = [[int(x) for x in row] for row in d]
    star = resampled_mdd(d, BR.bar_plan(len(d[0]), B, L, seed), exact)
    return records(d, star, levels, limits)


def assert_same(got, want, where, raw=True):
    """A DrawdownRisk against records(): every output, the first difference named."""
    for f in D.DD_LANE_DTYPE.names:
        g, w = got.lanes[f].reshape(-1), want.lanes[f].reshape(-1)
        bad = np.flatnonzero(g != w)
        assert not len(bad), f"{where}: {f} of lane {bad[0]}: {g[bad[0]]} against {w[bad[0]]}"
    for name in ("quantiles", "reach") + (("raw",) if raw else ()):
        g, w = getattr(got, name), getattr(want, name)
        w = w.reshape(g.shape)
        bad = np.argwhere(g != w)
        assert not len(bad), f"{where}: {name}{tuple(bad[0])}: {g[tuple(bad[0])]} against {w[tuple(bad[0])]}"


def out_bytes(r):
    return (r.lanes.tobytes(), r.quantiles.tobytes(), r.reach.tobytes(), None if r.raw is None else r.raw.tobytes())


# ------------------------------------------------------------------ what a case reaches
def anatomy(d, B, L, seed):
    """From the reference alone, per (lane, resample): the blocks' own drawdowns (each block walked
    by itself from a peak of 0) against MDD* of the whole path. Counts: `cross`: MDD* exceeds every
    block's own drawdown (peak and trough lie in different blocks); `single`: MDD* > 0 is some
    block's own; `wrapping`: ... a block's that wraps past bar T - 1."""
    T = len(d[0])
    lens = BR.blocks(T, L)
    starts = BR.starts(T, B, L, seed)
    out = dict(cross=0, single=0, wrapping=0, K=len(lens), last_differs=lens[-1] != lens[0])
    for row in d:
        for b in range(B):
            own, path = [], []
            for s, ln in zip(starts[b], lens):
                bars = [(s + u) % T for u in range(ln)]
                own.append((mdd(row[k] for k in bars), s + ln > T))
                path += bars
            whole = mdd(row[k] for k in path)
            best = max(x for x, _ in own)
            assert whole >= best
            out["cross"] += whole > best
            out["single"] += whole == best > 0
            out["wrapping"] += whole > 0 and any(x == whole and w for x, w in own)
    return out


# --------------------------------------------------------------------------- staged cases
OF_T = (1, 2, 63, 64, 65, 129)
OF_B = (1, 63, 64, 65, 255, 256, 257)
OF_N = (1, 3)
OF_SEED = 0xDD07


def of_L(T):
    """The block lengths of a staged T: 1, 2, T - 1, T, T + 5, 64, 65, those in [1, 2^22]."""
    return sorted({L for L in (1, 2, T - 1, T, T + 5, 64, 65) if L >= 1})


def of_rows(T, n):
    """n rows of T increments: a walk with a drift down, so that paths draw down across blocks, the
    second in thousands of ticks, the third mostly flat with rare large moves."""
    rng = np.random.default_rng([0xDD0F, T, n])
    rows = [rng.integers(-9, 8, T), rng.integers(-4000, 4001, T),
            np.where(rng.random(T) < 0.1, rng.integers(-10**6, 10**6, T), 0)]
    return np.array(rows[:n], np.int64)


@functools.lru_cache(None)
def of_cases(T):
    """[(L, B, n, seed)] of a staged T: every L with two sizes of B and n, every B and n with two L."""
    out = []
    for k, L in enumerate(of_L(T)):
        for B, n in ((OF_B[k % len(OF_B)], OF_N[k % 2]), (OF_B[(k + 3) % len(OF_B)], OF_N[(k + 1) % 2])):
            out.append((L, B, n, OF_SEED + 97 * T + k))
    for k, B in enumerate(OF_B):
        L = of_L(T)[(2 * k + 1) % len(of_L(T))]
        if (L, B) not in {(c[0], c[1]) for c in out}:
            out.append((L, B, OF_N[k % 2], OF_SEED + 97 * T + 50 + k))
    return tuple(out)


@functools.lru_cache(None)
def of_ref(T, k):
    L, B, n, seed = of_cases(T)[k]
    return drawdown_risk(of_rows(T, n).tolist(), B, L, seed)


def crafted():
    """{name: (rows, B, L, seed)}: rows whose MDD* is known in closed form or tied to the reality
    check."""
    T = 96
    dip = np.zeros(T, np.int64)
    dip[29:33] = (-5, -7, -3, -2)           # one dip over the edge of blocks of 10 and of 31 bars
    dip[60] = 4
    rng = np.random.default_rng(0xDD1B)
    return {
        "nonneg": (np.stack([rng.integers(0, 50, T), np.zeros(T, np.int64), np.full(T, 3)]), 65, 10, 1),
        "constant_neg": (np.stack([np.full(T, -7), np.full(T, -1), np.full(T, -BIG)]), 64, 7, 2),
        "nonpos": (np.stack([-rng.integers(0, 50, T), np.where(np.arange(T) % 5 == 0, -3, 0)]), 63, 10, 3),
        "dip": (np.stack([dip, -dip]), 255, 10, 4),
        "dip_31": (np.stack([dip, np.roll(dip, 40)]), 64, 31, 5),
        "rotation": (np.stack([rng.integers(-20, 21, T), dip]), 64, T, 6),       # L = T: one block, a rotation
        "rotation_above": (np.stack([rng.integers(-20, 21, T), dip]), 64, T + 5, 7),
    }


# ------------------------------------------------------------------------ walked cases
WALK_B = 40


def walk_params(strategy, seed):
    """(B, L, seed) of the walked case: block lengths below, at and above a tile, and one block."""
    k = RC.STRATEGIES.index(strategy) * 16 + seed
    return WALK_B, (10, 1, 64, 7, 65, 33, 10_000, 129)[seed % 8], 0xDD5EED + k


def lane_increments(strategy, seed, window=None):
    """[S * P][T] increments of every lane of random_cases.lane_case over the window (None: the
    default window), and (from, T)."""
    c, r = RC.lane_case(strategy, seed), RC.lane_refs(strategy, seed)
    frm, T = (0, max(c.bars)) if window is None else (window[0], window[1] - window[0])
    P = c.grid.n_params
    return [BR.increments(r.curves[s][p][1], c.bars[s], frm, T) for s in range(len(c.series)) for p in range(P)], (frm, T)


def cut_window(strategy, seed):
    """A window that starts inside the rows and ends past the shorter ones."""
    c = RC.lane_case(strategy, seed)
    second = sorted(c.bars)[-2]
    frm = min(70, second - 1)
    return frm, frm + 150


@functools.lru_cache(None)
def walk_ref(strategy, seed, cut=False):
    """(reference over every lane, window or None)."""
    window = cut_window(strategy, seed) if cut else None
    d, _ = lane_increments(strategy, seed, window)
    B, L, sd = walk_params(strategy, seed)
    return drawdown_risk(d, B, L, sd), window


EDGE = SimpleNamespace(B=16, L=5, seed=0xDDED)
EDGE_WINDOWS = ((0, 64), (63, 65), (64, 128), (1, 130), (128, 131), (129, 194), (699, 701), (700, 760))


@functools.lru_cache(None)
def edge_ref(strategy, frm, to):
    """The ragged rows of bootstrap_ref.edge_case (1, 2, 64, 65, 130 and 700 bars) over a window
    that starts or ends at a tile edge, or one bar past a row's end."""
    c = BR.edge_case(strategy)
    d = [BR.increments(eq, len(eq), frm, to - frm) for eq in c.curves]
    return drawdown_risk(d, EDGE.B, EDGE.L, EDGE.seed + 1000 * frm + to)


def _up(x):
    return (x + 255) // 256 * 256


def one_lane_budget(T, B, L, Q, R, lst, raw, row_mode, vals_lds, staged=False):
    """The staging budget under which plan_ddboot takes one lane per chunk, from the text of plan.h:
    what is held for the whole call, eight roundings, and one lane's staging with one byte to spare
    below a second lane's."""
    lp = min(L, T)
    K = -(-T // lp)
    two = K > 1 and T - (K - 1) * lp != lp
    row = (T + 1) * 8 + (2 if two else 1) * T * 24
    unit = (16 if lst else 0) + 72 + Q * 8 + R * 8 + (B * 8 if raw else 0) + (_up(row) if row_mode == 2 else 0) \
        + (0 if raw or vals_lds or Q == 0 else (B + 31) // 32 * 32 * 8) + ((T + 63) // 64 * 64 * 4 if staged else 0)
    return _up(K * B * 4) + _up(Q * 4) + _up(R * 8) + 8 * 256 + 2 * unit - 1
