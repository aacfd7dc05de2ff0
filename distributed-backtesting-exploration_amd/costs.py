"""Net of costs (docs/costs_spec.md): the binding of bt_costs, bt_set_costs_budget, bt_costs_host,
bt_costs_agg_host and bt_costs_merge, their two records and the result type. Engine.costs and
Engine.set_costs_budget (engine.py) forward here.

The two records are mirrored here and not in records.py, as overfit.py mirrors its own:
tests/test_abi_cpu.py checks every dtype of records.RECORDS against the layout that tests/abi_host.c
prints, and that program does not know these structs. tests/costs_abi_host.c prints theirs, and
tests/test_costs_cpu.py checks COST_RECORDS against it field by field in the same way."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from .engine import (_LATE_SYMBOLS, _check, _list_mode, _ptr, _ratio, _wide_f64, _wide_ints, as_lanes, sym)
from .records import TRADE_DTYPE

# one (lane, level) and one (parameter, level) of the net-of-costs call (docs/costs_spec.md)
COST_DTYPE = np.dtype([("n_trades", "<i4"), ("n_win", "<i4"), ("n_loss", "<i4"), ("n_bars", "<i4"),
                       ("mdd_bar", "<i4"), ("underwater_bars", "<i4"), ("pnl", "<i8"), ("fees", "<i8"),
                       ("turnover", "<i8"), ("mdd", "<i8"), ("win_sum", "<i8"), ("loss_sum", "<i8"),
                       ("s2_lo", "<u8"), ("s2_hi", "<i8")])
COST_AGG_DTYPE = np.dtype([("n_sym", "<i4"), ("n_traded", "<i4"), ("n_profit", "<i4"), ("pad", "<i4"),
                           ("trades", "<i8"), ("pnl", "<i8"), ("fees", "<i8"), ("mdd_max", "<i8")])
COST_RECORDS = {"bt_cost_rec": COST_DTYPE, "bt_cost_agg": COST_AGG_DTYPE}
assert [d.itemsize for d in COST_RECORDS.values()] == [88, 48]
COSTS_MAX = 1 << 20           # lanes per call in list mode
COST_LEVELS_MAX = 16
COST_FIXED_MAX = 1 << 20
COST_BPS_MAX = 1000

# bound on first use like every late entry point (engine.sym)
_LATE_SYMBOLS.update({
    "bt_costs": (3, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int32),
    "bt_set_costs_budget": (3, [C.c_void_p, C.c_int64], C.c_int32),
    "bt_costs_host": (3, [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p], C.c_int32),
    "bt_costs_agg_host": (3, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p], C.c_int32),
    "bt_costs_merge": (3, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p], C.c_int32),
})


def as_levels(levels) -> np.ndarray:
    """int32[C, 2]: the (fixed_ticks, bps) pairs of a call. The ranges are the library's to refuse;
    values that do not fit int32 are refused here."""
    a = np.asarray(list(levels) if not isinstance(levels, np.ndarray) else levels)
    if a.size == 0:
        return np.zeros((0, 2), np.int32)
    if a.ndim != 2 or a.shape[1] != 2 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("levels: a sequence of (fixed_ticks, bps) integer pairs")
    if a.min() < -2**31 or a.max() >= 2**31:
        raise ValueError("levels: the values are int32")
    return np.ascontiguousarray(a, np.int32)


@dataclass
class Costs:
    """Engine.costs' result (bt_costs, docs/costs_spec.md): every lane, and / or every parameter
    over all symbols, under each fee level. The derived figures are doubles, each 0 where its
    denominator is 0."""
    levels: np.ndarray            # int32[C, 2]: (fixed_ticks, bps)
    lanes: np.ndarray | None      # COST_DTYPE[n, C] (list mode, request order) or [S, P, C], when asked for
    params: np.ndarray | None     # COST_AGG_DTYPE[P, C], when asked for

    def _lanes(self) -> np.ndarray:
        if self.lanes is None:
            raise ValueError("costs: the per-lane records were not asked for")
        return self.lanes

    def _params(self) -> np.ndarray:
        if self.params is None:
            raise ValueError("costs: the per-parameter aggregates were not asked for")
        return self.params

    @property
    def s2(self) -> np.ndarray:
        """The sum of squared net increments of every (lane, level) as Python ints."""
        r = self._lanes()
        return _wide_ints(r["s2_lo"], r["s2_hi"])

    def net_sharpe(self, annualization: int = 252) -> np.ndarray:
        """sharpe_ticks of docs/portfolio_spec.md on the net increments: m = pnl / n_bars,
        v = s2 / n_bars - m m, (m / sqrt(v)) sqrt(annualization) where v > 0, else 0."""
        r = self._lanes()
        n = r["n_bars"].astype(np.float64)
        m = _ratio(r["pnl"], n)
        v = _ratio(_wide_f64(r["s2_lo"], r["s2_hi"]), n) - m * m
        ok = v > 0
        return np.where(ok, _ratio(m, np.sqrt(np.where(ok, v, 1.0))) * np.sqrt(float(annualization)), 0.0)

    def win_rate(self) -> np.ndarray:
        r = self._lanes()
        return _ratio(r["n_win"], r["n_trades"])

    def profit_factor(self) -> np.ndarray:
        r = self._lanes()
        return _ratio(r["win_sum"], r["loss_sum"])

    def breakeven_fixed(self) -> np.ndarray:
        """(pnl + fees) / (2 n_trades): the fixed fee per fill, in ticks, that zeroes the lane."""
        r = self._lanes()
        return _ratio(r["pnl"] + r["fees"], 2 * r["n_trades"].astype(np.int64))

    def breakeven_bps(self) -> np.ndarray:
        """(pnl + fees) 10000 / turnover: the proportional fee that zeroes the lane, ignoring the
        floor of every fill's fee (the true figure is a little higher)."""
        r = self._lanes()
        return _ratio((r["pnl"] + r["fees"]).astype(np.float64) * 10000.0, r["turnover"])

    def survivors(self) -> np.ndarray:
        """[P, C]: the share of symbols on which the parameter stays profitable at the level."""
        a = self._params()
        return _ratio(a["n_profit"], a["n_sym"])

    def rank(self, level: int, k: int | None = None) -> np.ndarray:
        """Parameter indices by total net pnl at `level`, best first, ties to the lower index."""
        a = self._params()
        if not 0 <= level < a.shape[1]:
            raise ValueError(f"costs: level {level} outside [0, {a.shape[1]})")
        order = np.argsort(-a["pnl"][:, level].astype(object), kind="stable").astype(np.int64)
        return order if k is None else order[:k]


def costs_host(trades, equity, levels) -> np.ndarray:
    """bt_costs_host: one lane's COST_DTYPE[C] from its complete trade list (TRADE_DTYPE), its gross
    equity curve, one value per bar, and the levels, on the CPU (no GPU needed): the scalar
    restatement of Engine.costs."""
    tr = np.ascontiguousarray(trades if trades is not None else np.zeros(0, TRADE_DTYPE), TRADE_DTYPE).reshape(-1)
    eq = np.ascontiguousarray(equity, np.int64)
    if eq.ndim != 1:
        raise ValueError("equity: one value per bar")
    lv = as_levels(levels)
    out = np.zeros(max(len(lv), 1), COST_DTYPE)
    _check(sym("bt_costs_host")(len(tr), tr.ctypes.data if len(tr) else None, len(eq), eq.ctypes.data if len(eq) else None,
                                len(lv), lv.ctypes.data if len(lv) else None, out.ctypes.data))
    return out[:len(lv)]


def costs_agg_host(recs) -> np.ndarray:
    """bt_costs_agg_host: an S x P x C array of COST_DTYPE records reduced over its rows to
    COST_AGG_DTYPE[P, C] on the CPU (no GPU needed)."""
    m = np.ascontiguousarray(recs, COST_DTYPE)
    if m.ndim != 3:
        raise ValueError("recs: an S x P x C array of COST_DTYPE")
    S, P, Cn = m.shape
    out = np.zeros(max(P * Cn, 1), COST_AGG_DTYPE)
    _check(sym("bt_costs_agg_host")(S, P, Cn, m.ctypes.data if m.size else None, out.ctypes.data))
    return out[:P * Cn].reshape(P, Cn)


def merge_costs(parts) -> np.ndarray:
    """bt_costs_merge: the aggregates (COST_AGG_DTYPE[P, C], or Costs with params) of disjoint row
    sets (shards, ranks) as one."""
    parts = [p.params if isinstance(p, Costs) else p for p in parts]
    if not parts or any(p is None or p.ndim != 2 for p in parts):
        raise ValueError("merge_costs: one COST_AGG_DTYPE[P, C] array per part")
    shape = parts[0].shape
    if any(p.shape != shape for p in parts):
        raise ValueError("merge_costs: the parts hold different parameter or level counts")
    block = np.ascontiguousarray(np.concatenate([p.reshape(-1) for p in parts]), COST_AGG_DTYPE)
    n = shape[0] * shape[1]
    out = np.zeros(max(n, 1), COST_AGG_DTYPE)
    _check(sym("bt_costs_merge")(block.ctypes.data, len(parts), n, out.ctypes.data))
    return out[:n].reshape(shape)


def engine_costs(engine, levels, lanes=None, per_lane: bool = True, params: bool = False) -> Costs:
    """Engine.costs."""
    f = sym("bt_costs")
    lv = as_levels(levels)
    Cn = len(lv)
    lvp = lv.ctypes.data if Cn else None
    if lanes is not None:
        if params:
            raise ValueError("costs: params aggregates every lane of the dataset; leave lanes out")
        req = as_lanes(lanes)
        n = len(req)
        out = np.zeros(max(n * Cn, 1), COST_DTYPE)
        keep = _list_mode(req)
        _check(f(engine._h, Cn, lvp, n, keep.ctypes.data, out.ctypes.data, None))
        return Costs(lv, out[:n * Cn].reshape(n, Cn), None)
    S, P = engine.stats()["n_symbols"], engine.n_params
    out = np.zeros(max(S * P * Cn, 1), COST_DTYPE) if per_lane else None
    agg = np.zeros(max(P * Cn, 1), COST_AGG_DTYPE) if params else None
    _check(f(engine._h, Cn, lvp, 0, None, _ptr(out), _ptr(agg)))
    return Costs(lv, None if out is None else out[:S * P * Cn].reshape(S, P, Cn),
                 None if agg is None else agg[:P * Cn].reshape(P, Cn))


def engine_set_costs_budget(engine, nbytes: int) -> None:
    _check(sym("bt_set_costs_budget")(engine._h, nbytes))
