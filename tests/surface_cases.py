"""Adversarial summary matrices for the surface tests (tests only; CPU and GPU tests share them).
No run produces these values, so they are the only way to drive the reductions to their limits:
clamped and tied Sharpes, .5 rounding ties of the fixed-point form, int128 carries, big pnl."""
import functools

import numpy as np

from surface_ref import SUMMARY, surface_ref

SHAPES = ((0, 3), (1, 1), (2, 65), (65, 12), (300, 7))

TINY = 5e-324
# sharpe * 2^32 exactly on a .5 tie: (k + 0.5) / 2^32 for even, odd, negative and large k
HALF_TIES = tuple((k + 0.5) / 2.0**32 for k in (0, 1, 2, 3, -1, -2, -3, 2**40 + 1, 2**40 + 2, -(2**46) - 1))
POOL = (0.0, -0.0, TINY, -TINY, 1e-300, -1e-300, 32768.0, -32768.0, 1e9, -1e9, 32767.999999999996,
        1.25, 1.25, -0.75, 2.5, 2.5, 2.5) + HALF_TIES


@functools.lru_cache(None)
def adversarial(S, P, seed=0x5AFE):
    """(summaries SUMMARY[S, P], ids int32[S]) with ids unique and unsorted."""
    rng = np.random.default_rng([seed, S, P])
    m = np.zeros((S, P), SUMMARY)
    pick = rng.integers(0, len(POOL), (S, P))
    sh = np.array(POOL)[pick]
    loose = rng.random((S, P)) < 0.25
    sh[loose] = rng.normal(0.0, 3.0, (S, P))[loose]
    if P > 1:   # one column far below zero (ss1 negative), one row of equal Sharpes
        sh[:, 0] = np.array((-32768.0, -1e9, -30000.5, -12345.678))[rng.integers(0, 4, S)]
    if S > 1:
        sh[S // 2, :] = 2.5
    m["sharpe"] = sh
    m["n_trades"] = rng.integers(0, 1000, (S, P)) * (rng.random((S, P)) < 0.8)
    m["status"] = np.where(rng.random((S, P)) < 0.05, -1, 0)
    big = rng.integers(-(2**52), 2**52, (S, P))
    edge = rng.random((S, P)) < 0.2
    big[edge] = np.where(rng.random((S, P)) < 0.5, 2**52 - 1, -(2**52) + 1)[edge]
    m["pnl"] = big * (rng.random((S, P)) < 0.9)
    m["mdd"] = rng.integers(0, 2**50, (S, P))
    m["exposure"] = rng.integers(0, 2**22, (S, P))
    m["hash"] = rng.integers(0, 2**63, (S, P)).astype(np.uint64) * 2 + 1
    ids = rng.permutation(np.concatenate([1 + rng.choice(2**31 - 3, max(S - 2, 0), replace=False),
                                          [0, 2**31 - 1]]).astype(np.int64))[:S].astype(np.int32)
    assert len(np.unique(ids)) == S
    m.setflags(write=False)
    ids.setflags(write=False)
    return m, ids


@functools.lru_cache(None)
def adversarial_ref(S, P):
    """surface_ref of adversarial(S, P): computed once, shared, left unchanged."""
    m, ids = adversarial(S, P)
    params, best = surface_ref(m, ids)
    params.setflags(write=False)
    best.setflags(write=False)
    return params, best


def assert_same(got, want, where):
    """Byte-for-byte equality of two record arrays, naming the first differing record and field."""
    assert got.dtype.itemsize == want.dtype.itemsize and got.shape == want.shape, (where, got.shape, want.shape)
    if got.tobytes() == want.tobytes():
        return
    g = got.view(want.dtype)
    for i in range(len(want)):
        if g[i].tobytes() != want[i].tobytes():
            diff = {f: (g[i][f], want[i][f]) for f in want.dtype.names if g[i][f].tobytes() != want[i][f].tobytes()}
            raise AssertionError(f"{where}: record {i} differs (got, want): {diff}")
