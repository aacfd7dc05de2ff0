"""Tail risk (docs/tail_spec.md): the binding of bt_tail, bt_tail_of, bt_tail_host, bt_set_tail_row,
bt_set_tail_budget and bt_last_tail_row, their two records and the result type. Engine.tail_risk,
Engine.tail_of, Engine.set_tail_row, Engine.set_tail_budget and Engine.last_tail_row (engine.py)
forward here.

The two records are mirrored here and not in records.py, as costs.py mirrors its own:
tests/tail_abi_host.c prints their layout, and tests/test_tail_cpu.py checks TAIL_RECORDS against it
field by field."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from statistics import NormalDist

import numpy as np

from .engine import (_LATE_SYMBOLS, _as_curves, _as_increments, _check, _list_mode, _ptr, _wide_ints, _window, as_lanes,
                     sym)

# one lane and one (lane, level) of the tail-risk call (docs/tail_spec.md)
TAIL_DTYPE = np.dtype([("n", "<i4"), ("n_window", "<i4"), ("n_pos", "<i4"), ("n_neg", "<i4"), ("min_bar", "<i4"),
                       ("max_bar", "<i4"), ("min_d", "<i8"), ("max_d", "<i8"), ("s1", "<i8"), ("s1_neg", "<i8"),
                       ("s2_lo", "<u8"), ("s2_hi", "<i8"), ("s2_neg_lo", "<u8"), ("s2_neg_hi", "<i8"),
                       ("s3_lo", "<u8"), ("s3_hi", "<i8"), ("s4", "<u8", (3,))])
TAIL_Q_DTYPE = np.dtype([("var", "<i8"), ("es_sum", "<i8"), ("k", "<i4"), ("n_lt", "<i4")])
TAIL_RECORDS = {"bt_tail_rec": TAIL_DTYPE, "bt_tail_q": TAIL_Q_DTYPE}
assert [d.itemsize for d in TAIL_RECORDS.values()] == [128, 24]
TAIL_MAX = 1 << 20            # lanes per call in list mode, rows of tail_of
TAIL_LEVELS_MAX = 8
TAIL_PPM_MAX = 1_000_000
TAIL_BARS_MAX = 1 << 22
TAIL_ALL, TAIL_HELD = 0, 1

# bound on first use like every late entry point (engine.sym)
_LATE_SYMBOLS.update({
    "bt_tail": (3, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                    C.c_void_p, C.c_void_p], C.c_int32),
    "bt_tail_of": (3, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p],
                   C.c_int32),
    "bt_tail_host": (3, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                         C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int32),
    "bt_set_tail_row": (3, [C.c_void_p, C.c_int32], C.c_int32),
    "bt_set_tail_budget": (3, [C.c_void_p, C.c_int64], C.c_int32),
    "bt_last_tail_row": (3, [C.c_void_p], C.c_int32),
})


def as_levels_ppm(levels) -> np.ndarray:
    """int32[Q]: the tail levels of a call in parts per million. Fractions (floats) become
    round(x * 10^6); integers are taken as ppm. The range is the library's to refuse; values that
    do not fit int32 are refused here."""
    out = []
    for x in (levels.tolist() if isinstance(levels, np.ndarray) else list(levels)):
        if isinstance(x, bool) or not isinstance(x, (int, float)):
            raise ValueError("levels: fractions (floats) or integer parts per million")
        v = round(x * 1_000_000) if isinstance(x, float) else x
        if not -2**31 <= v < 2**31:
            raise ValueError("levels: the values are int32")
        out.append(v)
    return np.array(out, np.int32)


def _isqrt_ratio(num: int, den: int) -> float:
    """sqrt(num / den) of non-negative Python ints, 0 where den is 0: the division is Python's
    correctly rounded int / int, then one sqrt."""
    return math.sqrt(num / den) if den > 0 else 0.0


def _sign(x: int) -> float:
    return (x > 0) - (x < 0)


def _phi(x: float) -> float:
    return 0.5 * (1.0 + math.erf(x / math.sqrt(2.0)))


@dataclass
class TailRisk:
    """Engine.tail_risk's result (bt_tail, docs/tail_spec.md): per lane the counts, extremes and
    exact power sums of its per-bar pnl increments d_t over the counted bars, and per (lane, level)
    the lower-tail order statistics. The derived views are plain Python on the exact integers in
    the order docs/tail_spec.md §6 fixes, each 0 where its denominator is 0. They are moments of
    tick increments, as the portfolio's and the covariance's are, and do not compare with
    bt_summary.sharpe, which is a Sharpe of per-bar returns."""
    levels_ppm: np.ndarray        # int32[Q]
    lanes: np.ndarray             # TAIL_DTYPE[n] (list mode, request order) or [S, P]
    quantiles: np.ndarray         # TAIL_Q_DTYPE[..., Q]

    @property
    def s2(self) -> np.ndarray:
        return _wide_ints(self.lanes["s2_lo"], self.lanes["s2_hi"])

    @property
    def s2_neg(self) -> np.ndarray:
        return _wide_ints(self.lanes["s2_neg_lo"], self.lanes["s2_neg_hi"])

    @property
    def s3(self) -> np.ndarray:
        return _wide_ints(self.lanes["s3_lo"], self.lanes["s3_hi"])

    @property
    def s4(self) -> np.ndarray:
        w = self.lanes["s4"].reshape(-1, 3).tolist()
        return np.array([a | (b << 64) | (c << 128) for a, b, c in w], object).reshape(self.lanes.shape)

    def _central(self):
        """[(n, s1, M2, M3, M4)] per lane, flat, as exact Python ints."""
        r = self.lanes.reshape(-1)
        out = []
        for n, s1, s2, s3, s4 in zip(r["n"].tolist(), r["s1"].tolist(), self.s2.reshape(-1), self.s3.reshape(-1),
                                     self.s4.reshape(-1)):
            out.append((n, s1, n * s2 - s1 * s1, n * n * s3 - 3 * n * s1 * s2 + 2 * s1 ** 3,
                        n ** 3 * s4 - 4 * n * n * s1 * s3 + 6 * n * s1 * s1 * s2 - 3 * s1 ** 4))
        return out

    def _view(self, f) -> np.ndarray:
        return np.array([f(*m) for m in self._central()], np.float64).reshape(self.lanes.shape)

    def mean(self) -> np.ndarray:
        return self._view(lambda n, s1, M2, M3, M4: s1 / n if n else 0.0)

    def std(self) -> np.ndarray:
        return self._view(lambda n, s1, M2, M3, M4: math.sqrt(M2) / n if n else 0.0)

    def skew(self) -> np.ndarray:
        return self._view(lambda n, s1, M2, M3, M4: _sign(M3) * _isqrt_ratio(M3 * M3, M2 ** 3))

    def kurtosis(self) -> np.ndarray:
        return self._view(lambda n, s1, M2, M3, M4: M4 / (M2 * M2) if M2 else 0.0)

    def sharpe(self, annualization: int = 1) -> np.ndarray:
        root = math.sqrt(float(annualization))
        return self._view(lambda n, s1, M2, M3, M4: _sign(s1) * _isqrt_ratio(s1 * s1, M2) * root)

    def sortino(self, annualization: int = 1) -> np.ndarray:
        root = math.sqrt(float(annualization))
        r = self.lanes.reshape(-1)
        vals = [_sign(s1) * _isqrt_ratio(s1 * s1, n * dn) * root
                for n, s1, dn in zip(r["n"].tolist(), r["s1"].tolist(), self.s2_neg.reshape(-1))]
        return np.array(vals, np.float64).reshape(self.lanes.shape)

    def gain_to_pain(self) -> np.ndarray:
        r = self.lanes.reshape(-1)
        vals = [s1 / -neg if neg else 0.0 for s1, neg in zip(r["s1"].tolist(), r["s1_neg"].tolist())]
        return np.array(vals, np.float64).reshape(self.lanes.shape)

    def var(self, j: int) -> np.ndarray:
        """The value at risk at level j as a loss: -var."""
        return -self.quantiles[..., j]["var"].astype(np.float64)

    def es(self, j: int) -> np.ndarray:
        """The expected shortfall at level j as a loss: -es_sum / k."""
        q = self.quantiles[..., j].reshape(-1)
        vals = [-s / k if k else 0.0 for s, k in zip(q["es_sum"].tolist(), q["k"].tolist())]
        return np.array(vals, np.float64).reshape(self.lanes.shape)

    def psr(self, sr0=0.0) -> np.ndarray:
        """The probabilistic Sharpe ratio against the per-bar threshold sr0 (a scalar or an array
        of the lanes' shape): Phi((SR - sr0) sqrt(n - 1) / sqrt(1 - skew SR + (kurtosis - 1) / 4
        SR^2)), SR the per-bar sharpe(1); 0 where n < 2, where the increments do not vary (M2 = 0) or
        where the radicand is not positive."""
        sr, sk, ku = self.sharpe(1).reshape(-1), self.skew().reshape(-1), self.kurtosis().reshape(-1)
        thr = np.broadcast_to(np.asarray(sr0, np.float64), self.lanes.shape).reshape(-1)
        out = []
        for (n, _, M2, _, _), s, g3, g4, t in zip(self._central(), sr.tolist(), sk.tolist(), ku.tolist(), thr.tolist()):
            den = 1.0 - g3 * s + (g4 - 1.0) / 4.0 * s * s
            out.append(_phi((s - t) * math.sqrt(n - 1) / math.sqrt(den)) if n >= 2 and M2 > 0 and den > 0 else 0.0)
        return np.array(out, np.float64).reshape(self.lanes.shape)

    def deflated_sharpe(self, n_trials=None, sr_var=None) -> np.ndarray:
        """psr at the threshold sqrt(V) ((1 - g) Z(1 - 1/N) + g Z(1 - 1/(N e))), g the
        Euler-Mascheroni constant, the expected best of N trials whose Sharpes have variance V. In
        all-lanes mode the defaults are per symbol: N = P and V the population variance of that
        symbol's P per-bar Sharpes; in list mode both arguments are required."""
        if self.lanes.ndim != 2 and (n_trials is None or sr_var is None):
            raise ValueError("deflated_sharpe: n_trials and sr_var are required in list mode")
        N = self.lanes.shape[-1] if n_trials is None else int(n_trials)
        if N < 2:
            raise ValueError(f"deflated_sharpe: n_trials = {N} is below 2")
        if sr_var is None:
            sr = self.sharpe(1)
            V = np.array([sum((x - sum(row) / len(row)) ** 2 for x in row) / len(row) for row in sr.tolist()])[:, None]
        else:
            V = np.asarray(sr_var, np.float64)
        g, Z = 0.5772156649015329, NormalDist().inv_cdf
        return self.psr(np.sqrt(V) * ((1.0 - g) * Z(1.0 - 1.0 / N) + g * Z(1.0 - 1.0 / (N * math.e))))


def _outputs(shape, Q):
    n = int(np.prod(shape))
    return np.zeros(max(n, 1), TAIL_DTYPE), np.zeros(max(n * Q, 1), TAIL_Q_DTYPE)


def _result(lv, recs, q, shape) -> TailRisk:
    n, Q = int(np.prod(shape)), len(lv)
    return TailRisk(lv, recs[:n].reshape(shape), q[:n * Q].reshape(*shape, Q))


def engine_tail_risk(engine, levels=(0.01, 0.05), lanes=None, window=None, held: bool = False) -> TailRisk:
    """Engine.tail_risk."""
    lv = as_levels_ppm(levels)
    frm, to = _window(window)
    mode = TAIL_HELD if held else TAIL_ALL
    lvp = lv.ctypes.data if len(lv) else None
    if lanes is not None:
        req = as_lanes(lanes)
        shape = (len(req),)
        recs, q = _outputs(shape, len(lv))
        _check(sym("bt_tail")(engine._h, len(req), _list_mode(req).ctypes.data, frm, to, mode, len(lv), lvp,
                              recs.ctypes.data, q.ctypes.data))
        return _result(lv, recs, q, shape)
    shape = (engine.stats()["n_symbols"], engine.n_params)
    recs, q = _outputs(shape, len(lv))
    _check(sym("bt_tail")(engine._h, 0, None, frm, to, mode, len(lv), lvp, recs.ctypes.data, q.ctypes.data))
    return _result(lv, recs, q, shape)


def engine_tail_of(engine, d, levels=(0.01, 0.05)) -> TailRisk:
    """Engine.tail_of."""
    a = _as_increments(d, "tail_of")
    lv = as_levels_ppm(levels)
    n, T = a.shape
    recs, q = _outputs((n,), len(lv))
    _check(sym("bt_tail_of")(engine._h, n, T, a.ctypes.data if a.size else None, len(lv),
                             lv.ctypes.data if len(lv) else None, recs.ctypes.data, q.ctypes.data))
    return _result(lv, recs, q, (n,))


def tail_risk_host(equity, pos, n_bars, levels=(0.01, 0.05), window=None, held: bool = False) -> TailRisk:
    """bt_tail_host: the scalar restatement of Engine.tail_risk on the CPU (no GPU needed) from
    replayed curves: Replay.equity, Replay.pos and Replay.n_bars of Engine.replay(curves=True);
    pos may be None unless held."""
    if pos is None:
        eq, nb = _as_curves(equity, n_bars)
        ps = None
    else:
        eq, nb, ps = _as_curves(equity, n_bars, pos)
    lv = as_levels_ppm(levels)
    frm, to = _window(window)
    n = eq.shape[0]
    recs, q = _outputs((n,), len(lv))
    _check(sym("bt_tail_host")(n, eq.ctypes.data if eq.size else None, _ptr(ps), nb.ctypes.data if n else None,
                               eq.shape[1], frm, to, TAIL_HELD if held else TAIL_ALL, len(lv),
                               lv.ctypes.data if len(lv) else None, recs.ctypes.data, q.ctypes.data))
    return _result(lv, recs, q, (n,))


def engine_set_tail_row(engine, mode: int) -> None:
    _check(sym("bt_set_tail_row")(engine._h, mode))


def engine_set_tail_budget(engine, nbytes: int) -> None:
    _check(sym("bt_set_tail_budget")(engine._h, nbytes))


def engine_last_tail_row(engine) -> int:
    return _check(sym("bt_last_tail_row")(engine._h))
