"""Probability of backtest overfitting (docs/cscv_spec.md): the binding of bt_cscv, bt_cscv_of and
bt_cscv_host, their two records and the result type. Engine.cscv (engine.py) forwards here.

The two records are mirrored here and not in records.py: tests/test_abi_cpu.py checks every dtype of
records.RECORDS against the layout that tests/abi_host.c prints, and that program does not know
these structs. tests/cscv_abi_host.c prints theirs, and tests/test_cscv_cpu.py checks CSCV_RECORDS
against it field by field in the same way."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from .engine import (_LATE_SYMBOLS, BtError, _as_bounds, _as_ids, _check, _ptr, _ratio, sym)
from .records import CSCV_MAX_FOLDS, CSCV_PICKS_MAX, FOLD_DTYPE

# one group's counts and one combination's pick of the probability of backtest overfitting
# (docs/cscv_spec.md)
CSCV_GROUP_DTYPE = np.dtype([("sym", "<i4"), ("n_lanes", "<i4"), ("n_live", "<i4"), ("n_dead", "<i4"),
                             ("n_overfit", "<i4"), ("n_loss", "<i4"), ("n_tied", "<i4"), ("pad", "<i4")])
CSCV_PICK_DTYPE = np.dtype([("lane", "<i4"), ("r2", "<i4"), ("is_sharpe", "<f8"), ("oos_sharpe", "<f8")])
CSCV_RECORDS = {"bt_cscv_group": CSCV_GROUP_DTYPE, "bt_cscv_pick": CSCV_PICK_DTYPE}
assert [d.itemsize for d in CSCV_RECORDS.values()] == [32, 24]

# bound on first use like every late entry point (engine.sym)
_LATE_SYMBOLS.update({
    "bt_cscv": (3, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int32),
    "bt_cscv_of": (3, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                       C.c_void_p], C.c_int32),
    "bt_cscv_host": (3, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                         C.c_void_p], C.c_int32),
})


def cscv_combos(K: int) -> np.ndarray:
    """uint32[C]: the masks of the C = binom(K, K/2) combinations of docs/cscv_spec.md in combination
    order, bit k set = fold k in-sample: every K-bit word with K/2 bits, ascending."""
    if K < 2 or K > CSCV_MAX_FOLDS or K % 2:
        raise ValueError(f"cscv: K = {K}, an even fold count in [2, {CSCV_MAX_FOLDS}]")
    w = np.arange(1 << K, dtype=np.uint32)
    bits = sum((w >> k) & 1 for k in range(K))
    return np.ascontiguousarray(w[bits == K // 2])


@dataclass
class Overfit:
    """Engine.cscv's result (bt_cscv, docs/cscv_spec.md): per group (dataset row) how often the lane
    that is best on one half of the folds ranks in the lower half on the other."""
    K: int
    groups: np.ndarray            # CSCV_GROUP_DTYPE[G]
    hist: np.ndarray | None       # uint32[G, 2P - 1]: live combinations per rank r2
    picks: np.ndarray | None      # CSCV_PICK_DTYPE[G, C], in combination order
    combos: np.ndarray            # uint32[C]: every combination's in-sample folds as a mask

    def pbo(self) -> np.ndarray:
        """Per group the probability of backtest overfitting: n_overfit / n_live (0 without a live
        combination)."""
        return _ratio(self.groups["n_overfit"], self.groups["n_live"])

    def prob_loss(self) -> np.ndarray:
        """Per group the share of live combinations whose pick loses out of sample."""
        return _ratio(self.groups["n_loss"], self.groups["n_live"])

    def _P(self) -> int:
        if self.hist is None:
            raise ValueError("cscv: hist was not asked for")
        return (self.hist.shape[1] + 1) // 2

    def omega(self) -> np.ndarray:
        """[2P - 1]: the relative rank of every bin of hist, (r2 + 2) / (2 (P + 1)), in (0, 1)."""
        P = self._P()
        return (np.arange(2 * P - 1, dtype=np.float64) + 2.0) / (2.0 * (P + 1))

    def logits(self) -> np.ndarray:
        """[2P - 1]: log(omega / (1 - omega)) of every bin of hist; at most 0 = overfit."""
        w = self.omega()
        return np.log(w / (1.0 - w))

    def degradation(self) -> np.ndarray:
        """[G, 2]: per group the least-squares slope and intercept of the picks' out-of-sample Sharpe
        on their in-sample Sharpe over the live combinations (0, 0 where the in-sample Sharpe
        has no spread)."""
        if self.picks is None:
            raise ValueError("cscv: picks were not asked for")
        out = np.zeros((len(self.groups), 2))
        for g, pk in enumerate(self.picks):
            pk = pk[pk["lane"] >= 0]
            if not len(pk):
                continue
            x, y = pk["is_sharpe"], pk["oos_sharpe"]
            dx = x - x.mean()
            den = float(dx @ dx)
            if den != 0:
                out[g, 0] = float(dx @ (y - y.mean())) / den
                out[g, 1] = y.mean() - out[g, 0] * x.mean()
        return out


def _as_folds(folds) -> np.ndarray:
    f = np.ascontiguousarray(folds, FOLD_DTYPE)
    if f.ndim != 3:
        raise ValueError("folds: a G x P x K array of FOLD_DTYPE")
    return f


def _cscv_bufs(G, P, K, hist, picks):
    """(groups, hist, picks, combos) of a call; K outside the range leaves one spare pick."""
    ok = 2 <= K <= CSCV_MAX_FOLDS and K % 2 == 0
    combos = cscv_combos(K) if ok else np.zeros(0, np.uint32)
    if picks and G * len(combos) > CSCV_PICKS_MAX:
        raise BtError(f"cscv: G*C = {G}*{len(combos)} exceeds 2^22 pick records")
    return (np.zeros(max(G, 1), CSCV_GROUP_DTYPE), np.zeros((max(G, 1), 2 * max(P, 1) - 1), np.uint32) if hist else None,
            np.zeros((max(G, 1), max(len(combos), 1)), CSCV_PICK_DTYPE) if picks else None, combos)


def _cscv_result(K, G, bufs) -> Overfit:
    grp, h, pk, combos = bufs
    return Overfit(K, grp[:G], None if h is None else h[:G], None if pk is None else pk[:G], combos)


def cscv_host(folds, sym_ids=None, annualization: int = 252, hist: bool = True, picks: bool = False) -> Overfit:
    """bt_cscv_host: the probability of backtest overfitting from fold records [G, P, K] on the CPU
    (no GPU needed), the scalar restatement of Engine.cscv."""
    f = _as_folds(folds)
    G, P, K = f.shape
    ids = None if sym_ids is None else _as_ids(sym_ids, G)
    bufs = _cscv_bufs(G, P, K, hist, picks)
    _check(sym("bt_cscv_host")(G, P, K, f.ctypes.data if f.size else None, _ptr(ids), annualization,
                               bufs[0].ctypes.data, _ptr(bufs[1]), _ptr(bufs[2])))
    return _cscv_result(K, G, bufs)


def engine_cscv(engine, bounds=None, folds=None, sym_ids=None, hist: bool = True, picks: bool = False) -> Overfit:
    """Engine.cscv: the walked form with `bounds`, the staged form with `folds` (exactly one)."""
    if (bounds is None) == (folds is None):
        raise ValueError("cscv: exactly one of bounds and folds")
    if bounds is not None:
        if sym_ids is not None:
            raise ValueError("cscv: sym_ids come with folds; with bounds the groups are the dataset's symbols")
        b = _as_bounds(bounds)
        K, G, P = len(b) - 1, engine.stats()["n_symbols"], engine.n_params
        bufs = _cscv_bufs(G, P, K, hist, picks)
        _check(sym("bt_cscv")(engine._h, K, b.ctypes.data if len(b) else None, bufs[0].ctypes.data, _ptr(bufs[1]),
                              _ptr(bufs[2])))
    else:
        f = _as_folds(folds)
        G, P, K = f.shape
        ids = None if sym_ids is None else _as_ids(sym_ids, G)
        bufs = _cscv_bufs(G, P, K, hist, picks)
        _check(sym("bt_cscv_of")(engine._h, G, P, K, f.ctypes.data if f.size else None, _ptr(ids),
                                 bufs[0].ctypes.data, _ptr(bufs[1]), _ptr(bufs[2])))
    return _cscv_result(K, G, bufs)
