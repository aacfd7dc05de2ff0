"""Drawdown bootstrap (docs/drawdown_spec.md): the binding of bt_drawdown_boot, bt_drawdown_boot_of,
bt_drawdown_boot_host, bt_set_ddboot_row, bt_set_ddboot_budget and bt_last_ddboot_row, the lane
record and the result type. Engine.drawdown_risk, Engine.drawdown_of, Engine.set_ddboot_row,
Engine.set_ddboot_budget and Engine.last_ddboot_row (engine.py) forward here.

The record is mirrored here and not in records.py, as tail.py mirrors its own:
tests/ddboot_abi_host.c prints its layout, and tests/test_ddboot_cpu.py checks DD_RECORDS against it
field by field."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

from .engine import (BOOT_MAX, BOOT_MAX_RESAMPLES, _LATE_SYMBOLS, _as_curves, _as_increments, _check, _list_mode, _ptr,
                     _u64, _wide_ints, _window, as_lanes, sym)
from .tail import as_levels_ppm

# one lane of the drawdown bootstrap (docs/drawdown_spec.md)
DD_LANE_DTYPE = np.dtype([("sum", "<i8"), ("mdd", "<i8"), ("n_ge", "<i8"), ("min_star", "<i8"), ("max_star", "<i8"),
                          ("m1_lo", "<u8"), ("m1_hi", "<i8"), ("m2_lo", "<u8"), ("m2_hi", "<i8")])
DD_RECORDS = {"bt_dd_lane": DD_LANE_DTYPE}
assert DD_LANE_DTYPE.itemsize == 72
DD_LEVELS_MAX = 8
DD_LIMITS_MAX = 8

_TAIL = [C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
         C.c_void_p]              # B, L, seed, Q, alpha_ppm, R, limits, lanes_out, q_out, reach_out, raw_out
# bound on first use like every late entry point (engine.sym)
_LATE_SYMBOLS.update({
    "bt_drawdown_boot": (3, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, *_TAIL], C.c_int32),
    "bt_drawdown_boot_of": (3, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, *_TAIL], C.c_int32),
    "bt_drawdown_boot_host": (3, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, *_TAIL], C.c_int32),
    "bt_set_ddboot_row": (3, [C.c_void_p, C.c_int32], C.c_int32),
    "bt_set_ddboot_budget": (3, [C.c_void_p, C.c_int64], C.c_int32),
    "bt_last_ddboot_row": (3, [C.c_void_p], C.c_int32),
})


def as_limits(limits) -> np.ndarray:
    """int64[R]: the loss limits of a call in ticks. The sign is the library's to refuse; values
    that do not fit int64 are refused here."""
    out = []
    for x in (limits.tolist() if isinstance(limits, np.ndarray) else list(limits)):
        if isinstance(x, bool) or not isinstance(x, int):
            raise ValueError("limits: integer ticks")
        if not -2**63 <= x < 2**63:
            raise ValueError("limits: the values are int64")
        out.append(x)
    return np.array(out, np.int64)


@dataclass
class DrawdownRisk:
    """Engine.drawdown_risk's result (bt_drawdown_boot, docs/drawdown_spec.md): per lane the
    observed largest drawdown and the distribution of the largest drawdown MDD* over `resamples`
    circular block resamples of its per-bar pnl increments. Every stored figure is an exact integer
    in ticks; the views are each one division or root on Python ints."""
    levels_ppm: np.ndarray        # int32[Q]
    limits: np.ndarray            # int64[R]
    resamples: int                # B
    lanes: np.ndarray             # DD_LANE_DTYPE[n] (list mode, request order) or [S, P]
    quantiles: np.ndarray         # int64[..., Q]: the ceil(B alpha)-th smallest MDD*
    reach: np.ndarray             # int64[..., R]: resamples with MDD* >= limit
    raw: np.ndarray | None        # int64[n, B]: the raw MDD*

    @property
    def m1(self) -> np.ndarray:
        return _wide_ints(self.lanes["m1_lo"], self.lanes["m1_hi"])

    @property
    def m2(self) -> np.ndarray:
        return _wide_ints(self.lanes["m2_lo"], self.lanes["m2_hi"])

    def mean(self) -> np.ndarray:
        """The mean MDD*: m1 / B."""
        B = self.resamples
        return np.array([a / B for a in self.m1.reshape(-1)], np.float64).reshape(self.lanes.shape)

    def std(self) -> np.ndarray:
        """The standard deviation of MDD*: the root of (B m2 - m1^2) / B^2, formed in Python ints."""
        B = self.resamples
        var = [B * b - a * a for a, b in zip(self.m1.reshape(-1), self.m2.reshape(-1))]
        return np.array([math.sqrt(v / (B * B)) if v > 0 else 0.0 for v in var], np.float64).reshape(self.lanes.shape)

    def p_value(self) -> np.ndarray:
        """n_ge / B: how often a resampled path draws down at least as deep as the observed one."""
        return np.array([g / self.resamples for g in self.lanes["n_ge"].reshape(-1).tolist()],
                        np.float64).reshape(self.lanes.shape)

    def quantile(self, j: int) -> np.ndarray:
        """The drawdown at level j in ticks, as a double."""
        return self.quantiles[..., j].astype(np.float64)

    def prob_reach(self) -> np.ndarray:
        """reach / B per lane and limit: the chance of a drawdown of at least the limit."""
        vals = [c / self.resamples for c in self.reach.reshape(-1).tolist()]
        return np.array(vals, np.float64).reshape(self.reach.shape)

    def pnl_to_dd(self, j: int) -> np.ndarray:
        """sum / quantile j per lane, 0 where the quantile is 0."""
        q = self.quantiles[..., j].reshape(-1).tolist()
        vals = [s / d if d else 0.0 for s, d in zip(self.lanes["sum"].reshape(-1).tolist(), q)]
        return np.array(vals, np.float64).reshape(self.lanes.shape)


def _args(resamples, block, seed, levels, limits, raw, n):
    """The shared tail of the three calls' arguments and the buffers behind it."""
    lv, lm = as_levels_ppm(levels), as_limits(limits)
    B = int(resamples)
    Bb = B if 0 < B <= BOOT_MAX_RESAMPLES else 0   # a refused B sizes no buffer
    Q, R = len(lv), len(lm)
    recs = np.zeros(max(n, 1), DD_LANE_DTYPE)
    q = np.zeros(max(n * Q, 1), np.int64)
    reach = np.zeros(max(n * R, 1), np.int64)
    rw = np.zeros(max(n * Bb, 1), np.int64) if raw else None
    args = (B, int(block), _u64(seed), Q, lv.ctypes.data if Q else None, R, lm.ctypes.data if R else None,
            recs.ctypes.data, q.ctypes.data, reach.ctypes.data, _ptr(rw))
    return args, (lv, lm, B, recs, q, reach, rw)


def _result(bufs, shape) -> DrawdownRisk:
    lv, lm, B, recs, q, reach, rw = bufs
    n, Q, R = int(np.prod(shape)), len(lv), len(lm)
    return DrawdownRisk(lv, lm, B, recs[:n].reshape(shape), q[:n * Q].reshape(*shape, Q), reach[:n * R].reshape(*shape, R),
                        None if rw is None else rw[:n * B].reshape(n, B))


def engine_drawdown_risk(engine, lanes=None, resamples: int = 1000, block: int = 10, seed: int = 0, window=None,
                         levels=(0.5, 0.95), limits=(), raw: bool = False) -> DrawdownRisk:
    """Engine.drawdown_risk."""
    frm, to = (0, 0) if window is None else _window(window)
    if lanes is None:
        if raw:
            raise ValueError("drawdown_risk: raw comes with lanes only")
        shape = (engine.stats()["n_symbols"], engine.n_params)
        args, bufs = _args(resamples, block, seed, levels, limits, False, int(np.prod(shape)))
        _check(sym("bt_drawdown_boot")(engine._h, 0, None, frm, to, *args))
        return _result(bufs, shape)
    req = as_lanes(lanes)
    args, bufs = _args(resamples, block, seed, levels, limits, raw, len(req))
    _check(sym("bt_drawdown_boot")(engine._h, len(req), _list_mode(req).ctypes.data, frm, to, *args))
    return _result(bufs, (len(req),))


def engine_drawdown_of(engine, d, resamples: int = 1000, block: int = 10, seed: int = 0, levels=(0.5, 0.95), limits=(),
                       raw: bool = False) -> DrawdownRisk:
    """Engine.drawdown_of."""
    a = _as_increments(d, "drawdown_of")
    n, T = a.shape
    args, bufs = _args(resamples, block, seed, levels, limits, raw, n if n <= BOOT_MAX else 0)
    _check(sym("bt_drawdown_boot_of")(engine._h, n, T, a.ctypes.data if a.size else None, *args))
    return _result(bufs, (n,))


def drawdown_risk_host(equity, n_bars, resamples: int = 1000, block: int = 10, seed: int = 0, window=None,
                       levels=(0.5, 0.95), limits=(), raw: bool = False) -> DrawdownRisk:
    """bt_drawdown_boot_host: the scalar restatement of Engine.drawdown_risk on the CPU (no GPU
    needed) from replayed curves (Replay.equity and Replay.n_bars of Engine.replay(curves=True)): it
    adds the drawn bars one by one and walks every resampled path."""
    eq, nb = _as_curves(equity, n_bars)
    n, stride = eq.shape
    frm, to = (0, 0) if window is None else _window(window)
    args, bufs = _args(resamples, block, seed, levels, limits, raw, n)
    _check(sym("bt_drawdown_boot_host")(n, eq.ctypes.data if eq.size else None, nb.ctypes.data if n else None, stride,
                                        frm, to, *args))
    return _result(bufs, (n,))


def engine_set_ddboot_row(engine, mode: int) -> None:
    _check(sym("bt_set_ddboot_row")(engine._h, mode))


def engine_set_ddboot_budget(engine, nbytes: int) -> None:
    _check(sym("bt_set_ddboot_budget")(engine._h, nbytes))


def engine_last_ddboot_row(engine) -> int:
    return _check(sym("bt_last_ddboot_row")(engine._h))
