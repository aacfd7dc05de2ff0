"""Reference for the covariance tests (tests only), written from docs/covariance_spec.md.

A lane's E_t comes from the C oracle's complete trade list through
replay_ref.curves_from_trades; the increments and every sum are Python ints. It shares nothing
with csrc/covariance.cpp or the kernels. Closed forms for the crafted matrices of bt_gram_of follow.

The cases the CPU and the GPU tests share are built once per process and must not be modified."""
import functools

import numpy as np

import dbx_amd as D
import walkfwd_ref as R
from replay_ref import curves_from_trades

MASK = (1 << 64) - 1
WHOLE = 2**31 - 1
# the whole series, a window across a tile edge, one tile, the tail, an empty one
WINDOWS = ((0, WHOLE), (63, 65), (64, 128), (500, 1000), (5, 5))


def increments(eq, frm, to_c):
    """d_t for t in [frm, to_c) of a curve over its own bars: E_t - E_(t-1) below them, then 0."""
    B = len(eq)
    return [(int(eq[t]) - (int(eq[t - 1]) if t else 0)) if t < B else 0 for t in range(frm, to_c)]


def covariance(curves, window):
    """curves: the lanes' equity curves over their own bars. Returns (gram [n, n] object array of
    Python ints, sums int64[n], T)."""
    frm, to = window
    b_max = max((len(e) for e in curves), default=0)
    to_c = min(to, b_max)
    T = max(0, to_c - frm)
    rows = [increments(e, frm, frm + T) for e in curves]
    return product(rows), np.array([sum(r) for r in rows], np.int64), T


def product(rows):
    """The Gram matrix of integer rows in Python ints."""
    n = len(rows)
    g = np.empty((n, n), object)
    for i in range(n):
        for j in range(i, n):
            g[i, j] = g[j, i] = sum(a * b for a, b in zip(rows[i], rows[j]))
    return g


def wide(g):
    """A matrix of Python ints as WIDE_DTYPE records: the bytes the library returns."""
    out = np.zeros(g.shape, D.WIDE_DTYPE)
    for idx in np.ndindex(*g.shape):
        v = int(g[idx])
        out[idx] = (v & MASK, v >> 64)
    return out


def assert_equal(got, want, what):
    """A Covariance against (gram, sums, T), byte for byte."""
    g, s, T = want
    assert got.n_bars == T, f"{what}: T = {got.n_bars}, want {T}"
    assert got.sums.dtype == np.int64 and np.array_equal(got.sums, s), f"{what}: sums {got.sums} want {s}"
    w = wide(g)
    assert got.wide.dtype == D.WIDE_DTYPE and got.wide.shape == w.shape, f"{what}: {got.wide.shape} vs {w.shape}"
    if got.wide.tobytes() != w.tobytes():
        mine = got.gram
        bad = [idx for idx in np.ndindex(*g.shape) if int(mine[idx]) != int(g[idx])]
        i, j = bad[0]
        raise AssertionError(f"{what}: gram[{i}][{j}] = {mine[i, j]}, want {g[i, j]} ({len(bad)} entries differ)")


# ------------------------------------------------------------------------------ the edge case
@functools.lru_cache(None)
def edge_lanes(strategy):
    """(grid, lanes [(sym id, param)], curves [equity list]) on the walk-forward edge set
    (walkfwd_ref.edge_series: 9 symbols of 1 to 1,000 bars, 12 params): two lanes of every symbol,
    two more of the long rows, and one lane twice. 21 lanes: no multiple of 16."""
    grid, _, lanes = R.edge_case(strategy)
    series = R.edge_series()
    pick = [(s, p) for s in range(len(series)) for p in ((2 * s) % 12, (2 * s + 7) % 12)]
    pick += [(8, 5), (7, 3), (8, 4)]
    assert pick.count((8, 4)) == 2 and len(pick) == 21
    curves = []
    for s, p in pick:
        _, eq = curves_from_trades(series[s][2], lanes[s][p][1])
        curves.append(eq.tolist())
    return grid, [(R.EDGE_IDS[s], p) for s, p in pick], curves


@functools.lru_cache(None)
def edge_reference(strategy, window):
    return covariance(edge_lanes(strategy)[2], window)


def curve_arrays(curves, stride):
    """The curves as bt_replay returns them: (equity int64[n, stride], n_bars int32[n])."""
    eq = np.zeros((len(curves), stride), np.int64)
    nb = np.zeros(len(curves), np.int32)
    for i, e in enumerate(curves):
        eq[i, :len(e)], nb[i] = e, len(e)
    return eq, nb


# -------------------------------------------------------------------------- crafted matrices
PMAX = 2**31 - 1


def crafted(name, n=20, T=67, seed=7):
    """int32 [n, T] matrices that leave one term of the 16-bit split alone, or push it to its end:
    low   |d| < 2^15: h = 0, the LL accumulator alone;
    high  multiples of 2^16: l = 0, the HH accumulator alone;
    half  d = 0x8000 mod 2^16: l = -2^15 everywhere, h up to 2^15 (d = 0x7FFF8000);
    ends  d = +-(2^31 - 1): h = +-2^15, l = -+1;
    full  random over the whole domain (-2^31, 2^31), every entry distinct."""
    rng = np.random.default_rng(seed)
    if name == "low":
        return rng.integers(-2**15 + 1, 2**15, (n, T)).astype(np.int32)
    if name == "high":
        return (rng.integers(-2**15 + 1, 2**15, (n, T)) * 65536).astype(np.int32)
    if name == "half":
        d = rng.integers(-2**15, 2**15, (n, T)) * 65536 + 0x8000
        d[0, :] = 0x7FFF8000
        d[1, ::2] = 0x7FFF8000
        return d.astype(np.int32)
    if name == "ends":
        return np.where(rng.integers(0, 2, (n, T)) == 1, PMAX, -PMAX).astype(np.int32)
    assert name == "full"
    while True:
        d = rng.integers(-PMAX, PMAX + 1, (n, T))
        if len(np.unique(d)) == d.size:
            return d.astype(np.int32)


def gram_of_reference(d):
    """(gram, sums, T) of an integer matrix by the Python-int product."""
    rows = [[int(x) for x in r] for r in d]
    return product(rows), np.array([sum(r) for r in rows], np.int64), d.shape[1]


def constant_gram(n, T, v):
    """Closed form for d = v everywhere: every entry T v^2, every sum T v."""
    g = np.empty((n, n), object)
    g[:, :] = T * v * v
    return g, np.full(n, T * v, np.int64), T
