"""ctypes binding of libbt.so (include/bt.h) — the MI355X backtest engine.

This is the Python face of the C ABI that replaces the reference worker's job function
(/root/reference/src/worker/process.rs:13-29). Every result comes from the HIP kernels;
there is no CPU fallback: if libbt.so or a GPU is missing, constructing an Engine raises.
"""
from __future__ import annotations

import ctypes as C
import importlib.util
import os
import subprocess
import sys
from dataclasses import dataclass, field
from typing import Sequence

import numpy as np

# the dtypes and constants of include/bt.h: every name of records.py is a name of this module too
from .records import *  # noqa: F401,F403

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# BT_LIB (tuning aid): another in-tree build of the library under dev/, e.g. dev/prof.so (the
# profiling build, `make PROFILING=1`) or dev/base.so for an A/B; nothing outside the package
_bt_lib = os.path.normpath(os.environ.get("BT_LIB", "libbt.so"))
if _bt_lib.startswith("..") or os.path.isabs(_bt_lib):
    raise ImportError(f"BT_LIB={_bt_lib}: a path inside {PKG_DIR} (libbt.so or dev/NAME.so)")
LIB_PATH = os.path.join(PKG_DIR, _bt_lib)
CSRC = os.path.join(PKG_DIR, "csrc")


class BtError(RuntimeError):
    pass


class _Config(C.Structure):
    _fields_ = [
        ("strategy", C.c_int32),
        ("n_fast", C.c_int32), ("n_slow", C.c_int32),
        ("fast", C.POINTER(C.c_int32)), ("slow", C.POINTER(C.c_int32)),
        ("n_span", C.c_int32), ("n_ols", C.c_int32),
        ("span", C.POINTER(C.c_int32)), ("ols", C.POINTER(C.c_int32)),
        ("band_bps", C.c_int32),
        ("n_bwin", C.c_int32), ("n_k", C.c_int32), ("n_sl", C.c_int32), ("n_tp", C.c_int32),
        ("bwin", C.POINTER(C.c_int32)), ("k_num", C.POINTER(C.c_int32)),
        ("k_den", C.c_int32),
        ("sl_bps", C.POINTER(C.c_int32)), ("tp_bps", C.POINTER(C.c_int32)),
        ("annualization", C.c_int64),
        ("device", C.c_int32), ("topk", C.c_int32), ("flags", C.c_int32),
        ("host_threads", C.c_int32), ("trade_cap", C.c_int32),
        ("stream", C.c_void_p),
    ]


class _JobIn(C.Structure):
    _fields_ = [("id", C.c_char_p), ("file", C.c_void_p), ("len", C.c_size_t)]


class _JobOut(C.Structure):
    _fields_ = [("data", C.c_void_p), ("len", C.c_size_t), ("status", C.c_int32),
                ("n_bars", C.c_int32)]


class _BatchProfile(C.Structure):
    _fields_ = [("n_jobs", C.c_int64), ("n_failed", C.c_int64), ("payload_bytes", C.c_int64),
                ("payload_bytes_read", C.c_int64), ("bars", C.c_int64),
                ("host_ingest_ms", C.c_double), ("upload_ms", C.c_double),
                ("compute_ms", C.c_double), ("readback_ms", C.c_double),
                ("format_ms", C.c_double), ("total_ms", C.c_double)]


class _Stats(C.Structure):
    _fields_ = [("n_symbols", C.c_int64), ("n_params", C.c_int64), ("bar_evals", C.c_int64),
                ("trades", C.c_int64), ("errors", C.c_int64)]


_lib = None


def build(force: bool = False) -> str:
    """Compile libbt.so in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    if force or not os.path.exists(LIB_PATH):
        subprocess.run(["make", "-s", "-j8", "-C", CSRC], check=True)
    return LIB_PATH


def _one_hip_runtime():
    """libbt.so needs libamdhip64.so.7 by SONAME. PyTorch-ROCm loads its bundled HIP and HSA
    runtimes by path, so a process that loads libbt.so first and torch afterwards holds two HSA
    runtimes, and torch then finds no GPU ("No HIP GPUs are available"; measured on the MI355X,
    scripts/dev/torch_after_libbt.py). With torch installed, importing it first lets libbt.so bind
    torch's copy: one runtime per process, whatever the caller imports later."""
    if "torch" in sys.modules:
        return
    if importlib.util.find_spec("torch") is not None:
        import torch  # noqa: F401


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BtError(f"{LIB_PATH} missing: run __graft_entry__.build() (no CPU fallback)")
    _one_hip_runtime()
    L = C.CDLL(LIB_PATH)
    P = C.c_void_p
    L.bt_engine_create.argtypes = [C.POINTER(_Config), C.c_char_p, C.c_size_t]
    L.bt_engine_create.restype = P
    L.bt_engine_destroy.argtypes = [P]
    L.bt_engine_destroy.restype = None
    L.bt_last_error.restype = C.c_char_p
    L.bt_abi_version.restype = C.c_int32
    L.bt_num_params.argtypes = [P]
    L.bt_set_segments.argtypes = [P, C.c_int32, C.c_int32]
    L.bt_last_segments.argtypes = [P, C.POINTER(C.c_int64)]
    L.bt_run_batch.argtypes = [P, C.c_size_t, C.POINTER(_JobIn), C.POINTER(_JobOut)]
    L.bt_job_out_free.argtypes = [C.POINTER(_JobOut), C.c_size_t]
    L.bt_job_out_free.restype = None
    L.bt_load_synthetic.argtypes = [P, C.c_uint64, C.c_int64, C.c_int32, C.c_int32, C.c_int32]
    L.bt_load_ohlc.argtypes = [P, C.c_int32, P, P, P, P, P, P]
    for f in ("bt_run", "bt_sync", "bt_reset_timing"):
        getattr(L, f).argtypes = [P]
    L.bt_read_summaries.argtypes = [P, P, C.c_size_t]
    L.bt_read_sums.argtypes = [P, P, C.c_size_t]
    L.bt_read_trades.argtypes = [P, P, C.c_size_t]
    L.bt_read_topk.argtypes = [P, P, C.c_int32]
    L.bt_read_stats.argtypes = [P, C.POINTER(_Stats)]
    L.bt_topk_fetch_async.argtypes = [P, C.c_int32]
    L.bt_topk_fetch_wait.argtypes = [P, C.c_int32, P, C.c_int32, C.POINTER(C.c_int64)]
    L.bt_read_close.argtypes = [P, C.c_int32, P, C.c_int32]
    L.bt_kernel_timing.argtypes = [P, C.POINTER(C.c_double), C.POINTER(C.c_int64),
                                   C.POINTER(C.c_char_p)]
    L.bt_merge_topk.argtypes = [P, C.c_size_t, C.c_int32, P]
    L.bt_i128_to_double.argtypes = [C.c_uint64, C.c_int64]
    L.bt_i128_to_double.restype = C.c_double
    L.bt_parse_csv.argtypes = [C.c_char_p, C.c_size_t, C.c_int32, P, P, P, C.c_char_p,
                               C.c_size_t]
    L.bt_parse_job.argtypes = L.bt_parse_csv.argtypes
    L.bt_encode_columns.argtypes = [P, P, P, P, P, C.c_int32, P, C.c_size_t]
    L.bt_encode_columns.restype = C.c_int64
    L.bt_gen_payload.argtypes = [C.c_uint64, C.c_int64, C.c_int32, C.c_int32, P, C.c_size_t]
    L.bt_gen_payload.restype = C.c_int64
    L.bt_last_batch_profile.argtypes = [P, C.POINTER(_BatchProfile)]
    L.bt_format_summaries.argtypes = [P, C.c_int32, P, C.c_size_t]
    L.bt_format_summaries.restype = C.c_int64
    _lib = L
    return L


# Entry points added after ABI version 2 (the multi-GPU exchange), bound on first use: an older
# library (e.g. a previous round's build, loaded with BT_LIB for a regression check) then still
# loads and runs everything else. Each carries the first ABI version whose signature it matches:
# a symbol whose signature changed (bt_exchange_merge gained block_bytes in ABI 3) must not be
# bound with the new argument list on a library that exports the old one.
_LATE_SYMBOLS = {
    "bt_comm_unique_id": (2, [C.c_void_p], C.c_int32),
    "bt_comm_create": (2, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_char_p,
                           C.c_size_t], C.c_void_p),
    "bt_comm_destroy": (2, [C.c_void_p], None),
    "bt_exchange_async": (2, [C.c_void_p, C.c_void_p, C.c_int32], C.c_int32),
    "bt_exchange_wait": (2, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p], C.c_int32),
    "bt_exchange_message_bytes": (2, [C.c_int32], C.c_int64),
    "bt_exchange_merge": (3, [C.c_void_p, C.c_size_t, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                              C.c_void_p], C.c_int32),
    "bt_replay": (3, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64], C.c_int32),
    "bt_surface": (3, [C.c_void_p, C.c_void_p, C.c_void_p], C.c_int32),
    "bt_surface_of": (3, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                          C.c_void_p], C.c_int32),
    "bt_topk_of": (3, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                       C.c_void_p], C.c_int32),
    "bt_set_surface_chunks": (3, [C.c_void_p, C.c_int32], C.c_int32),
    "bt_surface_host": (3, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
                        C.c_int32),
    "bt_surface_merge": (3, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p], C.c_int32),
    "bt_walk_forward": (3, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                            C.c_void_p], C.c_int32),
    "bt_set_walkfwd_budget": (3, [C.c_void_p, C.c_int64], C.c_int32),
    "bt_walk_forward_host": (3, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                 C.c_int64, C.c_void_p, C.c_void_p], C.c_int32),
    "bt_set_cscv_work": (3, [C.c_void_p, C.c_int64], C.c_int32),
    "bt_portfolio": (3, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                         C.c_void_p, C.c_void_p], C.c_int32),
    "bt_set_portfolio_replicas": (3, [C.c_void_p, C.c_int32], C.c_int32),
    "bt_portfolio_host": (3, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32,
                              C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int32),
    "bt_portfolio_merge": (3, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int32),
    "bt_covariance": (3, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                          C.c_void_p], C.c_int32),
    "bt_gram_of": (3, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int32),
    "bt_set_gram_split": (3, [C.c_void_p, C.c_int32], C.c_int32),
    "bt_set_run_overlap": (3, [C.c_void_p, C.c_int32], C.c_int32),
    "bt_trade_stats": (3, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int32),
    "bt_set_tstats_budget": (3, [C.c_void_p, C.c_int64], C.c_int32),
    "bt_trade_stats_host": (3, [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p], C.c_int32),
    "bt_tstats_agg_host": (3, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p], C.c_int32),
    "bt_tstats_merge": (3, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p], C.c_int32),
    "bt_bootstrap": (3, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                         C.c_int32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int32),
    "bt_bootstrap_of": (3, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                            C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int32),
    "bt_set_boot_budget": (3, [C.c_void_p, C.c_int64], C.c_int32),
    "bt_set_boot_row": (3, [C.c_void_p, C.c_int32], C.c_int32),
    "bt_bootstrap_host": (3, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int32,
                              C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                              C.c_void_p], C.c_int32),
    "bt_covariance_host": (3, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p,
                               C.c_void_p, C.c_void_p], C.c_int32),
}
_late = {}


def sym(name: str):
    """A late (post-v2) entry point of libbt.so, typed on first use. BtError if the loaded
    library's ABI predates the signature bound here (or AttributeError if it lacks the symbol)."""
    f = _late.get(name)
    if f is None:
        min_abi, argtypes, restype = _LATE_SYMBOLS[name]
        have = lib().bt_abi_version()
        if have < min_abi:
            raise BtError(f"{name}: {LIB_PATH} has ABI {have}, this binding needs ABI >= {min_abi}")
        f = getattr(lib(), name)
        f.argtypes, f.restype = argtypes, restype
        _late[name] = f
    return f


def _check(rc):
    if rc < 0:
        raise BtError(lib().bt_last_error().decode())
    return rc


def _arr(v) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(v, dtype=np.int32))


def _ptr(a):
    """An optional array as a pointer argument: NULL for None."""
    return None if a is None else a.ctypes.data


def _list_mode(req) -> np.ndarray:
    """The lanes argument of a call in which lanes != NULL selects list mode: `req`, or one spare
    record when there is no request to point at."""
    return req if len(req) else np.zeros(1, LANE_DTYPE)


def _u64(seed) -> int:
    return int(seed) & (2**64 - 1)


def _wide_ints(lo, hi) -> np.ndarray:
    """int128 values given as arrays of their lo and hi words, as Python ints (an object array)."""
    vals = [(h << 64) | l for l, h in zip(lo.reshape(-1).tolist(), hi.reshape(-1).tolist())]
    return np.array(vals, object).reshape(lo.shape)


def _wide_f64(lo, hi) -> np.ndarray:
    """The same values as doubles, each through bt_i128_to_double: one rounding."""
    vals = [i128_to_double(l, h) for l, h in zip(lo.reshape(-1).tolist(), hi.reshape(-1).tolist())]
    return np.array(vals, np.float64).reshape(lo.shape)


def _as_ids(sym_ids, S) -> np.ndarray:
    ids = np.ascontiguousarray(np.asarray(sym_ids, np.int32))
    if ids.shape != (S,):
        raise ValueError(f"sym_ids: {S} ids for {S} rows, got shape {ids.shape}")
    return ids


def _as_curves(equity, n_bars, *pos):
    """The curves a *_host call takes (Replay.equity, Replay.n_bars and, where given, Replay.pos
    of Engine.replay(curves=True)): int64 [n, stride], int32 [n] and int8 [n, stride]."""
    eq = np.ascontiguousarray(equity, np.int64)
    ps = [np.ascontiguousarray(p, np.int8) for p in pos]
    nb = np.ascontiguousarray(np.asarray(n_bars, np.int32))
    if eq.ndim != 2 or any(p.shape != eq.shape for p in ps) or nb.shape != (eq.shape[0],):
        raise ValueError("equity and pos: n x stride arrays, n_bars: n bar counts" if pos
                         else "equity: an n x stride array, n_bars: n bar counts")
    return (eq, nb, *ps)


def _as_increments(d, who) -> np.ndarray:
    """The [n, T] increments of gram_of and bootstrap_of (`who`, for the message) as int32."""
    a = np.asarray(d)
    if a.ndim != 2 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{who}: an n x T integer array")
    if a.size and (a.min() < -2**31 or a.max() >= 2**31):
        raise ValueError(f"{who}: the increments are int32")
    return np.ascontiguousarray(a, np.int32)


@dataclass
class Grid:
    """Worker-side parameter grid (the proto carries none: SURVEY.md §7 hard part 5)."""
    strategy: int
    axes: Sequence[Sequence[int]]
    band_bps: int = 20
    k_den: int = 2
    annualization: int = 252
    _keep: list = field(default_factory=list, repr=False)

    @property
    def n_params(self) -> int:
        n = 1
        for a in self.axes:
            n *= len(a)
        return n

    @staticmethod
    def sma(fast, slow, annualization=252):
        return Grid(BT_SMA_CROSS, [list(fast), list(slow)], annualization=annualization)

    @staticmethod
    def ema_ols(span, ols, band_bps=20, annualization=98280):
        return Grid(BT_EMA_OLS, [list(span), list(ols)], band_bps=band_bps,
                    annualization=annualization)

    @staticmethod
    def boll(win, k_num, sl_bps, tp_bps, k_den=2, annualization=98280):
        return Grid(BT_BOLL, [list(win), list(k_num), list(sl_bps), list(tp_bps)], k_den=k_den,
                    annualization=annualization)

    def param(self, p: int) -> dict:
        """Decode a param index (include/bt.h ordering) into named values."""
        if self.strategy == BT_SMA_CROSS:
            return {"f": self.axes[0][p // len(self.axes[1])], "s": self.axes[1][p % len(self.axes[1])]}
        if self.strategy == BT_EMA_OLS:
            return {"n": self.axes[0][p // len(self.axes[1])], "w": self.axes[1][p % len(self.axes[1])],
                    "band_bps": self.band_bps}
        nk, nsl, ntp = (len(a) for a in self.axes[1:])
        return {"w": self.axes[0][p // (ntp * nsl * nk)], "k_num": self.axes[1][(p // (ntp * nsl)) % nk],
                "k_den": self.k_den, "sl": self.axes[2][(p // ntp) % nsl], "tp": self.axes[3][p % ntp]}

    def to_c(self, device=0, topk=0, flags=0, host_threads=0, trade_cap=0, stream=None) -> _Config:
        cfg = _Config()
        cfg.strategy = self.strategy
        arrs = [_arr(a) for a in self.axes]
        self._keep = arrs
        ptr = [a.ctypes.data_as(C.POINTER(C.c_int32)) for a in arrs]
        if self.strategy == BT_SMA_CROSS:
            cfg.n_fast, cfg.n_slow = len(arrs[0]), len(arrs[1])
            cfg.fast, cfg.slow = ptr
        elif self.strategy == BT_EMA_OLS:
            cfg.n_span, cfg.n_ols = len(arrs[0]), len(arrs[1])
            cfg.span, cfg.ols = ptr
            cfg.band_bps = self.band_bps
        else:
            cfg.n_bwin, cfg.n_k, cfg.n_sl, cfg.n_tp = (len(a) for a in arrs)
            cfg.bwin, cfg.k_num, cfg.sl_bps, cfg.tp_bps = ptr
            cfg.k_den = self.k_den
        cfg.annualization = self.annualization
        cfg.device, cfg.topk, cfg.flags = device, topk, flags
        cfg.host_threads, cfg.trade_cap = host_threads, trade_cap
        cfg.stream = stream
        return cfg


# Pinned grids of BASELINE.json configs.
def config2_grid():
    return Grid.sma(range(4, 43, 2), range(50, 241, 10), annualization=252)


def config3_grid():
    return Grid.ema_ols([10, 20, 30, 60, 120, 240, 390, 780],
                        [15, 30, 60, 120, 240, 390, 780, 1560], band_bps=20, annualization=98280)


def config4_grid():
    return Grid.boll([10, 20, 30, 45, 60, 90, 120, 240], [3, 4, 5, 6], [50, 100],
                     [50, 100, 200, 400], k_den=2, annualization=98280)


def config5_grid():
    # SMA fast 32 x slow 32 on 1-min bars
    return Grid.sma(range(5, 161, 5), range(200, 6401, 200), annualization=98280)


def as_lanes(lanes) -> np.ndarray:
    """The request array of Engine.replay (LANE_DTYPE[n]) from top-k records (TOPK_DTYPE: their
    sym and param fields), an (n, 2) integer array or a list of (sym, param) pairs."""
    a = lanes if isinstance(lanes, np.ndarray) else np.asarray(list(lanes))
    if a.dtype.names is not None:
        if not {"sym", "param"} <= set(a.dtype.names):
            raise ValueError("lane records need sym and param fields")
        a = a.reshape(-1)
    out = np.zeros(len(a), LANE_DTYPE)
    if a.dtype.names is not None:
        out["sym"], out["param"] = a["sym"], a["param"]
    elif len(a):
        if a.ndim != 2 or a.shape[1] != 2 or not np.issubdtype(a.dtype, np.integer):
            raise ValueError("lanes: top-k records, an (n, 2) integer array or a list of (sym, param) pairs")
        if a.min() < -2**31 or a.max() >= 2**31:
            raise ValueError("lanes: sym and param are int32")
        out["sym"], out["param"] = a[:, 0], a[:, 1]
    return out


@dataclass
class Replay:
    """Engine.replay's result, rows in request order."""
    lanes: np.ndarray       # LANE_DTYPE[n], the request
    summaries: np.ndarray   # SUMMARY_DTYPE[n]
    n_bars: np.ndarray      # int32[n], bars of each lane's symbol
    trades: np.ndarray | None   # TRADE_DTYPE[n, trade_cap]: the first trades, then zeros
    equity: np.ndarray | None   # int64[n, max bars]: E_t (spec §4), zero past the symbol's bars
    pos: np.ndarray | None      # int8[n, max bars]: position after bar t


@dataclass
class Surface:
    """A run reduced along each axis (bt_surface, docs/surface_spec.md): one aggregate per
    parameter over every symbol, and each symbol's best lane in dataset row order."""
    params: np.ndarray            # PARAM_AGG_DTYPE[P]
    best: np.ndarray | None       # TOPK_DTYPE[S] (feeds Engine.replay), or None when not asked for

    def _sum128(self, name) -> np.ndarray:
        return _wide_f64(self.params[name + "_lo"], self.params[name + "_hi"])

    def mean_sharpe(self) -> np.ndarray:
        """Mean over the symbols of the clamped fixed-point Sharpe (0.0 where n_sym == 0)."""
        n = self.params["n_sym"].astype(np.float64)
        return np.divide(self._sum128("ss1") / 2.0**32, n, out=np.zeros(len(n)), where=n > 0)

    def std_sharpe(self) -> np.ndarray:
        """Population standard deviation of the same, from ss1 and ss2."""
        n = self.params["n_sym"].astype(np.float64)
        m2 = np.divide(self._sum128("ss2") / 2.0**64, n, out=np.zeros(len(n)), where=n > 0)
        return np.sqrt(np.maximum(m2 - self.mean_sharpe() ** 2, 0.0))

    def win_rate(self) -> np.ndarray:
        """Share of the symbols with pnl > 0."""
        n = self.params["n_sym"].astype(np.float64)
        return np.divide(self.params["n_win"].astype(np.float64), n, out=np.zeros(len(n)), where=n > 0)

    def rank(self, k=None, by="mean_sharpe") -> np.ndarray:
        """Parameter indices, best (largest `by`) first, ties to the lower index; Grid.param
        decodes them. `by`: mean_sharpe, std_sharpe, win_rate or a numeric field of `params`."""
        derived = {"mean_sharpe": self.mean_sharpe, "std_sharpe": self.std_sharpe, "win_rate": self.win_rate}
        if by in derived:
            v = derived[by]()
        elif by in (self.params.dtype.names or ()):
            v = self.params[by]
        else:
            raise ValueError(f"rank by {by!r}: one of {sorted(derived)} or a field of PARAM_AGG_DTYPE")
        # descending and stable without negating (int64 minima, unsigned fields)
        order = (len(v) - 1 - np.argsort(v[::-1], kind="stable"))[::-1]
        return order if k is None else order[:k]


def _surface_bufs(S, P, best):
    agg = np.zeros(max(P, 1), PARAM_AGG_DTYPE)
    rec = np.zeros(max(S, 1), TOPK_DTYPE) if best else None
    return agg, rec


def _as_matrix(summaries, sym_ids):
    m = np.ascontiguousarray(summaries, SUMMARY_DTYPE)
    if m.ndim != 2:
        raise ValueError("summaries: an S x P array of SUMMARY_DTYPE")
    return m, _as_ids(sym_ids, m.shape[0])


def surface_host(summaries, sym_ids, best=True) -> Surface:
    """bt_surface_host: the reductions of an S x P summary matrix on the CPU (no GPU needed)."""
    m, ids = _as_matrix(summaries, sym_ids)
    S, P = m.shape
    agg, rec = _surface_bufs(S, P, best)
    _check(sym("bt_surface_host")(S, P, m.ctypes.data if m.size else None, ids.ctypes.data if S else None,
                                  agg.ctypes.data, _ptr(rec)))
    return Surface(agg[:P], None if rec is None else rec[:S])


def merge_surfaces(parts) -> Surface:
    """bt_surface_merge: surfaces of disjoint symbol sets (shards, ranks) as one. The per-symbol
    records are concatenated in the order given."""
    parts = list(parts)
    world = len(parts)
    P = len(parts[0].params) if parts else 0
    if any(len(s.params) != P for s in parts):
        raise ValueError("merge_surfaces: the surfaces hold different parameter counts")
    block = (np.ascontiguousarray(np.concatenate([s.params for s in parts]), PARAM_AGG_DTYPE) if parts
             else np.zeros(1, PARAM_AGG_DTYPE))
    out = np.zeros(max(P, 1), PARAM_AGG_DTYPE)
    _check(sym("bt_surface_merge")(block.ctypes.data, world, P, out.ctypes.data))
    best = (np.concatenate([s.best for s in parts]) if parts and all(s.best is not None for s in parts)
            else None)
    return Surface(out[:P], best)


@dataclass
class WalkForward:
    """Engine.walk_forward's result (bt_walk_forward, docs/walkforward_spec.md), rows in dataset
    row order."""
    bounds: np.ndarray | None     # int32[K + 1], the fold bounds (None from walk_forward_host)
    train: int                    # training folds per step (0 = anchored)
    steps: np.ndarray             # WF_STEP_DTYPE[S, n_steps]; Grid.param decodes steps["param"] >= 0
    total: np.ndarray             # FOLD_DTYPE[S]: each row's out-of-sample folds as one record
    folds: np.ndarray | None      # FOLD_DTYPE[S, P, K] when asked for

    def oos_sharpe(self) -> np.ndarray:
        """Per row, the Sharpe of its out-of-sample folds taken together (total["sharpe"])."""
        return self.total["sharpe"].copy()

    def train_sharpe(self) -> np.ndarray:
        """[S, n_steps]: the training Sharpe each step's parameter was chosen with (0 where none)."""
        return self.steps["train_sharpe"].copy()


def _as_bounds(bounds) -> np.ndarray:
    b = np.asarray(list(bounds) if not isinstance(bounds, np.ndarray) else bounds)
    if b.ndim != 1 or not np.issubdtype(b.dtype, np.integer) or (len(b) and (b.min() < -2**31 or b.max() >= 2**31)):
        raise ValueError("bounds: a 1-D sequence of int32 bar indices")
    return np.ascontiguousarray(b, np.int32)


def walk_forward_host(folds, sym_ids, train: int = 1, annualization: int = 252) -> WalkForward:
    """bt_walk_forward_host: the steps and totals from fold records [S, P, K] on the CPU (no GPU
    needed), the scalar restatement of Engine.walk_forward's selection."""
    f = np.ascontiguousarray(folds, FOLD_DTYPE)
    if f.ndim != 3:
        raise ValueError("folds: an S x P x K array of FOLD_DTYPE")
    S, P, K = f.shape
    ids = _as_ids(sym_ids, S)
    n_steps = max(K - max(train, 1), 0)
    steps = np.zeros((max(S, 1), max(n_steps, 1)), WF_STEP_DTYPE)
    total = np.zeros(max(S, 1), FOLD_DTYPE)
    _check(sym("bt_walk_forward_host")(S, P, K, train, f.ctypes.data if f.size else None,
                                       ids.ctypes.data if S else None, annualization, steps.ctypes.data,
                                       total.ctypes.data))
    steps = np.ascontiguousarray(steps.reshape(-1)[:S * n_steps]).reshape(S, n_steps)
    return WalkForward(None, train, steps, total[:S], f)


@dataclass
class Portfolio:
    """Engine.portfolio's result (bt_portfolio, docs/portfolio_spec.md): chosen lanes traded
    together, bar by bar."""
    pnl: np.ndarray               # int64[T]: the book's mark-to-market change over bar t, ticks
    equity: np.ndarray            # int64[T]: its running sum
    n_long: np.ndarray            # int32[T]: entries in window and long after bar t
    n_short: np.ndarray           # int32[T]
    summary: np.ndarray           # PF_SUMMARY_DTYPE, one record (shape ())
    annualization: int = 252      # of the Sharpe (merge_portfolios recomputes it)

    def gross(self) -> np.ndarray:
        """Positions held per bar: n_long + n_short."""
        return self.n_long + self.n_short

    def net(self) -> np.ndarray:
        """n_long - n_short."""
        return self.n_long - self.n_short


def as_pf_lanes(lanes, windows=None) -> np.ndarray:
    """The entry array of Engine.portfolio (PF_LANE_DTYPE[n]): `lanes` as PF_LANE_DTYPE records, or
    anything as_lanes accepts with `windows`, one (from_bar, to_bar) pair for every entry or an
    (n, 2) integer array; without windows every entry runs [0, 2^31 - 1)."""
    if isinstance(lanes, np.ndarray) and lanes.dtype == PF_LANE_DTYPE:
        if windows is not None:
            raise ValueError("windows: the PF_LANE_DTYPE entries carry their own")
        return np.ascontiguousarray(lanes.reshape(-1))
    req = as_lanes(lanes)
    out = np.zeros(len(req), PF_LANE_DTYPE)
    out["sym"], out["param"] = req["sym"], req["param"]
    out["to_bar"] = PF_WHOLE
    if windows is not None:
        w = np.asarray(windows)
        if not np.issubdtype(w.dtype, np.integer) or w.shape not in ((2,), (len(req), 2)):
            raise ValueError("windows: one (from_bar, to_bar) pair or an (n, 2) integer array")
        if w.size and (w.min() < -2**31 or w.max() >= 2**31):
            raise ValueError("windows: from_bar and to_bar are int32")
        w = np.broadcast_to(w, (len(req), 2))
        out["from_bar"], out["to_bar"] = w[:, 0], w[:, 1]
    return out


def walk_forward_lanes(wf: WalkForward) -> np.ndarray:
    """The portfolio entries of a walk-forward result: every step that chose a parameter, as
    (sym, param, oos.first_bar, oos.first_bar + oos.n_bars). Engine.portfolio of them is the
    out-of-sample book of the changing picks stitched together."""
    st = wf.steps.reshape(-1)
    st = st[st["param"] >= 0]
    out = np.zeros(len(st), PF_LANE_DTYPE)
    out["sym"], out["param"] = st["sym"], st["param"]
    out["from_bar"] = st["oos"]["first_bar"]
    out["to_bar"] = st["oos"]["first_bar"] + st["oos"]["n_bars"]
    return out


def _pf_bufs(T):
    T = max(int(T), 1)
    return (np.zeros(T, np.int64), np.zeros(T, np.int64), np.zeros(T, np.int32), np.zeros(T, np.int32),
            np.zeros(1, PF_SUMMARY_DTYPE))


def _pf_result(bufs, T, annualization) -> Portfolio:
    T = max(int(T), 0)
    pnl, eq, nl, ns, summ = bufs
    return Portfolio(pnl[:T], eq[:T], nl[:T], ns[:T], summ[0], int(annualization))


def portfolio_host(equity, pos, n_bars, windows=None, T=None, annualization: int = 252) -> Portfolio:
    """bt_portfolio_host: the portfolio of n entries from their curves (Replay.equity, Replay.pos
    and Replay.n_bars of Engine.replay(curves=True)) on the CPU (no GPU needed), the scalar
    restatement of Engine.portfolio. `windows` as in as_pf_lanes; T defaults to the longest entry."""
    eq, nb, ps = _as_curves(equity, n_bars, pos)
    n, stride = eq.shape
    req = as_pf_lanes(np.zeros((n, 2), np.int32), windows)
    if T is None:
        T = int(nb.max()) if n else 1
    bufs = _pf_bufs(T)
    _check(sym("bt_portfolio_host")(n, eq.ctypes.data if eq.size else None, ps.ctypes.data if ps.size else None,
                                    nb.ctypes.data if n else None, stride, req.ctypes.data if n else None, T,
                                    annualization, *(b.ctypes.data for b in bufs)))
    return _pf_result(bufs, T, annualization)


def merge_portfolios(parts) -> Portfolio:
    """bt_portfolio_merge: portfolios of disjoint entry sets over the same bars (shards, ranks) as
    one: the rows add, and equity and the summary are recomputed from the sums."""
    parts = list(parts)
    if not parts:
        raise ValueError("merge_portfolios: no parts")
    T, ann = len(parts[0].pnl), parts[0].annualization
    if any(len(p.pnl) != T or p.annualization != ann for p in parts):
        raise ValueError("merge_portfolios: the parts differ in their bars or annualization")
    pnl = np.ascontiguousarray(np.stack([p.pnl for p in parts]), np.int64)
    nl = np.ascontiguousarray(np.stack([p.n_long for p in parts]), np.int32)
    ns = np.ascontiguousarray(np.stack([p.n_short for p in parts]), np.int32)
    summ = np.ascontiguousarray(np.stack([p.summary for p in parts]), PF_SUMMARY_DTYPE)
    bufs = _pf_bufs(T)
    _check(sym("bt_portfolio_merge")(len(parts), T, pnl.ctypes.data, nl.ctypes.data, ns.ctypes.data, summ.ctypes.data,
                                     ann, *(b.ctypes.data for b in bufs)))
    return _pf_result(bufs, T, ann)


@dataclass
class Covariance:
    """Engine.covariance's result (bt_covariance, docs/covariance_spec.md): the exact Gram matrix
    of the lanes' per-bar pnl increments over one window, and what follows from it. The float
    methods work on gram_f64, each step a single IEEE double operation in the order written."""
    wide: np.ndarray              # WIDE_DTYPE[n, n]: the Gram matrix as the library returns it
    sums: np.ndarray              # int64[n]: the sum of each lane's increments
    n_bars: int                   # T, the bars of the window

    @property
    def gram(self) -> np.ndarray:
        """[n, n] Python ints."""
        return _wide_ints(self.wide["lo"], self.wide["hi"])

    @property
    def gram_f64(self) -> np.ndarray:
        """[n, n] doubles, every entry through bt_i128_to_double: one rounding."""
        return _wide_f64(self.wide["lo"], self.wide["hi"])

    def cov(self) -> np.ndarray:
        """gram_f64 / T - outer(sums / T, sums / T); zeros when the window has no bar."""
        n = len(self.sums)
        if self.n_bars < 1:
            return np.zeros((n, n))
        T = float(self.n_bars)
        m = self.sums.astype(np.float64) / T
        return self.gram_f64 / T - np.outer(m, m)

    def vol(self) -> np.ndarray:
        """The root of cov's diagonal, 0 where a variance is not positive."""
        v = np.diagonal(self.cov())
        return np.sqrt(np.where(v > 0, v, 0.0))

    def corr(self) -> np.ndarray:
        """cov over the root of the diagonal products, 0 where a variance is not positive."""
        c = self.cov()
        v = np.diagonal(c)
        ok = v > 0
        den = np.sqrt(np.outer(np.where(ok, v, 1.0), np.where(ok, v, 1.0)))
        return np.where(np.outer(ok, ok), c / den, 0.0)

    def book_s2(self, weights=None) -> int:
        """w^T gram w in Python ints, exact, for integer weights; all ones by default: the s2 of
        the portfolio of the same lanes over the same window."""
        n = len(self.sums)
        w = [1] * n if weights is None else [int(x) for x in weights]
        if len(w) != n or (weights is not None and any(int(x) != x for x in weights)):
            raise ValueError("book_s2: one integer weight per lane")
        g = self.gram
        return sum(w[i] * w[j] * g[i, j] for i in range(n) for j in range(n))


def _window(window):
    if window is None:
        return 0, PF_WHOLE
    w = np.asarray(window)
    if w.shape != (2,) or not np.issubdtype(w.dtype, np.integer) or w.min() < -2**31 or w.max() >= 2**31:
        raise ValueError("window: one (from_bar, to_bar) pair of int32")
    return int(w[0]), int(w[1])


def _cov_result(n, wide, sums, T) -> Covariance:
    return Covariance(wide[:n * n].reshape(n, n), sums[:n], int(T))


def covariance_host(equity, n_bars, window=None) -> Covariance:
    """bt_covariance_host: the covariance of n lanes from their replayed equity curves
    (Replay.equity and Replay.n_bars of Engine.replay(curves=True)) on the CPU (no GPU needed), the
    scalar restatement of Engine.covariance."""
    eq, nb = _as_curves(equity, n_bars)
    n, stride = eq.shape
    frm, to = _window(window)
    wide, sums, T = np.zeros(max(n * n, 1), WIDE_DTYPE), np.zeros(max(n, 1), np.int64), C.c_int32(0)
    _check(sym("bt_covariance_host")(n, eq.ctypes.data if eq.size else None, nb.ctypes.data if n else None, stride,
                                     frm, to, wide.ctypes.data, sums.ctypes.data, C.addressof(T)))
    return _cov_result(n, wide, sums, T.value)


@dataclass
class RealityCheck:
    """Engine.reality_check's result (bt_bootstrap, docs/bootstrap_spec.md): White's bootstrap
    reality check of the best lane of every group, over `resamples` circular block resamples of the
    lanes' per-bar pnl increments. Every stored figure is an exact integer."""
    groups: np.ndarray            # BOOT_GROUP_DTYPE[G]
    resamples: int                # B
    lanes: np.ndarray | None      # BOOT_LANE_DTYPE[n] (per_lane)
    vmax: np.ndarray | None       # int64[G, B]: V* of every group and resample (vmax)
    boot: np.ndarray | None       # int64[n, B]: the raw resampled sums (boot)

    def p_value(self) -> np.ndarray:
        """n_ge / B per group: how often the best centred resampled sum of the group reaches the
        observed best sum."""
        return self.groups["n_ge"].astype(np.float64) / float(self.resamples)

    def critical(self, q: float) -> np.ndarray:
        """Per group the smallest observed-best sum that would have had a p-value of at most
        1 - q: the ceil(q B)-th smallest V*, plus one tick (int64)."""
        if self.vmax is None:
            raise ValueError("reality_check: vmax was not asked for")
        if not 0.0 < q <= 1.0:
            raise ValueError("critical: q in (0, 1]")
        k = max(int(np.ceil(q * self.resamples)), 1)
        return np.sort(self.vmax, axis=1)[:, k - 1] + 1

    def _lanes(self) -> np.ndarray:
        if self.lanes is None:
            raise ValueError("reality_check: per_lane was not asked for")
        return self.lanes

    def lane_se(self) -> np.ndarray:
        """The bootstrap standard error of every lane's sum: the root of m2 / B - (m1 / B)^2,
        formed exactly as (B m2 - m1^2) / B^2 in Python ints and then rounded once."""
        r, B = self._lanes(), self.resamples
        m1, m2 = _wide_ints(r["m1_lo"], r["m1_hi"]), _wide_ints(r["m2_lo"], r["m2_hi"])
        var = [B * b - a * a for a, b in zip(m1.reshape(-1), m2.reshape(-1))]
        return np.array([float(np.sqrt(v / (B * B))) if v > 0 else 0.0 for v in var], np.float64).reshape(r.shape)

    def lane_p(self) -> np.ndarray:
        """n_nonpos / B per lane: how often a lane's resampled sum is not positive."""
        return self._lanes()["n_nonpos"].astype(np.float64) / float(self.resamples)


def _as_goff(groups, n):
    """Group sizes -> offsets (int32[G + 1]), or None for one group."""
    if groups is None:
        return None
    g = np.asarray(groups)
    if g.ndim != 1 or len(g) == 0 or not np.issubdtype(g.dtype, np.integer):
        raise ValueError("groups: a list of group sizes")
    if int(g.sum()) != n or g.min() < 0:
        raise ValueError(f"groups: the sizes add to {int(g.sum())}, the lanes number {n}")
    return np.ascontiguousarray(np.concatenate(([0], np.cumsum(g))), np.int32)


def _boot_bufs(n, G, B, per_lane, vmax, boot):
    return (np.zeros(max(G, 1), BOOT_GROUP_DTYPE), np.zeros(max(n, 1), BOOT_LANE_DTYPE) if per_lane else None,
            np.zeros(max(G * B, 1), np.int64) if vmax else None, np.zeros(max(n * B, 1), np.int64) if boot else None)


def _boot_result(bufs, n, G, B) -> RealityCheck:
    grp, rec, vm, bt_ = bufs
    return RealityCheck(grp[:G], B, None if rec is None else rec[:n], None if vm is None else vm[:G * B].reshape(G, B),
                        None if bt_ is None else bt_[:n * B].reshape(n, B))


def reality_check_host(equity, n_bars, groups=None, resamples: int = 1000, block: int = 10, seed: int = 0,
                       window=None, per_lane: bool = False, vmax: bool = False, boot: bool = False) -> RealityCheck:
    """bt_bootstrap_host: the reality check of n lanes from their replayed equity curves
    (Replay.equity and Replay.n_bars of Engine.replay(curves=True)) on the CPU (no GPU needed), the
    scalar restatement of Engine.reality_check: it adds the drawn bars one by one."""
    eq, nb = _as_curves(equity, n_bars)
    n, stride = eq.shape
    goff = _as_goff(groups, n)
    G = 1 if goff is None else len(goff) - 1
    frm, to = (0, 0) if window is None else _window(window)
    B = int(resamples)
    bufs = _boot_bufs(n, G, B if 0 < B <= BOOT_MAX_RESAMPLES else 0, per_lane, vmax, boot)
    _check(sym("bt_bootstrap_host")(n, eq.ctypes.data if eq.size else None, nb.ctypes.data if n else None, stride, G,
                                    _ptr(goff), frm, to, B, int(block), _u64(seed), *(_ptr(b) for b in bufs)))
    return _boot_result(bufs, n, G, B)


def _ratio(num, den) -> np.ndarray:
    """num / den in doubles, 0 where den is 0."""
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    return np.divide(num, den, out=np.zeros(np.broadcast(num, den).shape), where=den != 0)


@dataclass
class TradeStats:
    """Engine.trade_stats' result (bt_trade_stats, docs/tradestats_spec.md). The derived figures
    are doubles, each 0 where its denominator is 0, of the per-lane records, or of the
    per-parameter aggregates with params=True (and when there are no per-lane records)."""
    lanes: np.ndarray | None      # TSTATS_DTYPE[n] (list mode, request order) or [S, P], when asked for
    params: np.ndarray | None     # TSTATS_AGG_DTYPE[P], when asked for

    def _of(self, params) -> np.ndarray:
        r = self.params if params or self.lanes is None else self.lanes
        if r is None:
            raise ValueError("trade_stats: that output was not asked for")
        return r

    @staticmethod
    def _sq(r) -> np.ndarray:
        return _wide_ints(r["sq_lo"], r["sq_hi"])

    @property
    def sq(self) -> np.ndarray:
        """The sum of squared trade pnl as Python ints (of the aggregates when there are no
        per-lane records)."""
        return self._sq(self._of(False))

    @property
    def params_sq(self) -> np.ndarray:
        return self._sq(self._of(True))

    def win_rate(self, params=False) -> np.ndarray:
        r = self._of(params)
        return _ratio(r["n_win"], r["n_trades"])

    def profit_factor(self, params=False) -> np.ndarray:
        r = self._of(params)
        return _ratio(r["gross_win"], r["gross_loss"])

    def expectancy(self, params=False) -> np.ndarray:
        """The mean trade pnl, ticks."""
        r = self._of(params)
        return _ratio(r["gross_win"] - r["gross_loss"], r["n_trades"])

    def avg_win(self, params=False) -> np.ndarray:
        r = self._of(params)
        return _ratio(r["gross_win"], r["n_win"])

    def avg_loss(self, params=False) -> np.ndarray:
        r = self._of(params)
        return _ratio(r["gross_loss"], r["n_loss"])

    def payoff(self, params=False) -> np.ndarray:
        """avg_win over avg_loss."""
        return _ratio(self.avg_win(params), self.avg_loss(params))

    def avg_hold(self, params=False) -> np.ndarray:
        """Bars held per trade."""
        r = self._of(params)
        return _ratio(r["hold_sum"], r["n_trades"])

    def trade_std(self, params=False) -> np.ndarray:
        """Population standard deviation of the trade pnl, from sq and the mean."""
        r = self._of(params)
        sq = _wide_f64(r["sq_lo"], r["sq_hi"])
        return np.sqrt(np.maximum(_ratio(sq, r["n_trades"]) - self.expectancy(params) ** 2, 0.0))

    def t_stat(self, params=False) -> np.ndarray:
        """expectancy over its standard error trade_std / sqrt(n_trades)."""
        r = self._of(params)
        return _ratio(self.expectancy(params) * np.sqrt(r["n_trades"].astype(np.float64)), self.trade_std(params))


def trade_stats_host(trades, equity) -> np.ndarray:
    """bt_trade_stats_host: one lane's TSTATS_DTYPE record (shape ()) from its complete trade list
    in closing order (TRADE_DTYPE) and its equity curve, one value per bar, on the CPU (no GPU
    needed): the scalar restatement of Engine.trade_stats."""
    tr = np.ascontiguousarray(trades if trades is not None else np.zeros(0, TRADE_DTYPE), TRADE_DTYPE).reshape(-1)
    eq = np.ascontiguousarray(equity, np.int64)
    if eq.ndim != 1:
        raise ValueError("equity: one value per bar")
    out = np.zeros(1, TSTATS_DTYPE)
    _check(sym("bt_trade_stats_host")(len(tr), tr.ctypes.data if len(tr) else None, len(eq),
                                      eq.ctypes.data if len(eq) else None, out.ctypes.data))
    return out[0]


def trade_stats_agg_host(recs) -> np.ndarray:
    """bt_tstats_agg_host: an S x P matrix of TSTATS_DTYPE records reduced over its rows to
    TSTATS_AGG_DTYPE[P] on the CPU (no GPU needed)."""
    m = np.ascontiguousarray(recs, TSTATS_DTYPE)
    if m.ndim != 2:
        raise ValueError("recs: an S x P array of TSTATS_DTYPE")
    S, P = m.shape
    out = np.zeros(max(P, 1), TSTATS_AGG_DTYPE)
    _check(sym("bt_tstats_agg_host")(S, P, m.ctypes.data if m.size else None, out.ctypes.data))
    return out[:P]


def merge_trade_stats(parts) -> np.ndarray:
    """bt_tstats_merge: the aggregates (TSTATS_AGG_DTYPE[P], or TradeStats with params) of disjoint
    row sets (shards, ranks) as one."""
    parts = [p.params if isinstance(p, TradeStats) else p for p in parts]
    if not parts or any(p is None for p in parts):
        raise ValueError("merge_trade_stats: one TSTATS_AGG_DTYPE[P] array per part")
    P = len(parts[0])
    if any(len(p) != P for p in parts):
        raise ValueError("merge_trade_stats: the parts hold different parameter counts")
    block = np.ascontiguousarray(np.concatenate(parts), TSTATS_AGG_DTYPE)
    out = np.zeros(max(P, 1), TSTATS_AGG_DTYPE)
    _check(sym("bt_tstats_merge")(block.ctypes.data, len(parts), P, out.ctypes.data))
    return out[:P]


class Engine:
    """One engine per GPU (one process per GPU)."""

    def __init__(self, grid: Grid, device=0, topk=0, parity=False, timing=False,
                 trade_cap=0, host_threads=0, stream=None):
        self.grid = grid
        flags = (BT_FLAG_PARITY if parity else 0) | (BT_FLAG_TIMING if timing else 0)
        cfg = grid.to_c(device, topk, flags, host_threads, trade_cap, stream)
        err = C.create_string_buffer(512)
        h = lib().bt_engine_create(C.byref(cfg), err, 512)
        if not h:
            raise BtError(err.value.decode())
        self._h = h
        self.n_params = lib().bt_num_params(h)
        self.trade_cap = trade_cap
        self.n_symbols = 0
        self.topk = topk
        self._sym_bars = None  # bars by symbol id of the resident dataset, when loaded from here

    def close(self):
        if getattr(self, "_h", None):
            lib().bt_engine_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- HBM-resident path
    def load_synthetic(self, seed, sym_begin, n_sym, n_bars, freq=BT_DAILY):
        self._sym_bars = None
        _check(lib().bt_load_synthetic(self._h, seed & ((1 << 64) - 1), sym_begin, n_sym, n_bars, freq))
        self.n_symbols = n_sym
        self._sym_bars = (sym_begin, n_sym, n_bars)

    def load_ohlc(self, closes, highs=None, lows=None, sym_ids=None):
        """closes: list of 1-D int arrays (ragged allowed)."""
        bars = np.array([len(c) for c in closes], np.int32)
        offs = np.zeros(len(closes), np.int64)
        if len(closes):
            offs[1:] = np.cumsum(bars[:-1])
        cat = lambda xs: np.ascontiguousarray(np.concatenate([np.asarray(x, np.int32) for x in xs])) if len(xs) else np.zeros(1, np.int32)
        c = cat(closes)
        h = cat(highs) if highs is not None else None
        lo = cat(lows) if lows is not None else None
        ids = np.ascontiguousarray(np.arange(len(closes), dtype=np.int64) if sym_ids is None
                                   else np.asarray(sym_ids, np.int64))
        self._sym_bars = None
        _check(lib().bt_load_ohlc(self._h, len(closes), ids.ctypes.data, bars.ctypes.data,
                                  offs.ctypes.data, _ptr(h), _ptr(lo), c.ctypes.data))
        self.n_symbols = len(closes)
        # the engine keeps ids as int32; with a repeated id the first row wins (bt_replay)
        self._sym_bars = {}
        for i, b in zip(ids.astype(np.int32).tolist(), bars.tolist()):
            self._sym_bars.setdefault(i, b)

    def run(self):
        _check(lib().bt_run(self._h))

    def set_segments(self, segments: int, burn_tiles: int = 0) -> None:
        """Bar-axis split of the EMA+OLS / Bollinger walks: 0 = automatic, 1 = off, n = n
        segments per symbol; burn_tiles 0 = the strategy's default burn-in."""
        _check(lib().bt_set_segments(self._h, segments, burn_tiles))

    def set_run_overlap(self, on) -> None:
        """Consecutive runs on two streams in turn, a run's first blocks filling the compute units
        the run before it frees (bt_set_run_overlap; on by default). Results are identical either
        way; split runs, parity engines and engines on a caller's stream stay serial."""
        _check(sym("bt_set_run_overlap")(self._h, 1 if on else 0))

    def last_segments(self, with_refixed: bool = False):
        """Segments per symbol of the last run (and, with_refixed, the fix pass's re-walks)."""
        n = C.c_int64(0)
        g = _check(lib().bt_last_segments(self._h, C.byref(n)))
        return (g, int(n.value)) if with_refixed else g

    def sync(self):
        _check(lib().bt_sync(self._h))

    def summaries(self) -> np.ndarray:
        n = self.n_symbols * self.n_params
        out = np.zeros(max(n, 1), SUMMARY_DTYPE)
        _check(lib().bt_read_summaries(self._h, out.ctypes.data, n))
        return out[:n].reshape(self.n_symbols, self.n_params)

    def sums(self) -> np.ndarray:
        n = self.n_symbols * self.n_params
        out = np.zeros(max(n, 1), SUMS_DTYPE)
        _check(lib().bt_read_sums(self._h, out.ctypes.data, n))
        return out[:n].reshape(self.n_symbols, self.n_params)

    def trades(self) -> np.ndarray:
        n = self.n_symbols * self.n_params * self.trade_cap
        out = np.zeros(max(n, 1), TRADE_DTYPE)
        _check(lib().bt_read_trades(self._h, out.ctypes.data, n))
        return out[:n].reshape(self.n_symbols, self.n_params, self.trade_cap)

    def read_topk(self, k=None) -> np.ndarray:
        k = k or self.topk
        out = np.zeros(k, TOPK_DTYPE)
        m = _check(lib().bt_read_topk(self._h, out.ctypes.data, k))
        return out[:m]

    def topk_fetch_async(self, slot: int) -> None:
        """Enqueue the read-back of the last run's top-k and trade count into pinned slot
        0 .. PIPE_SLOTS-1 (no host wait): later runs can be enqueued before these records are
        consumed."""
        _check(lib().bt_topk_fetch_async(self._h, slot))

    def topk_fetch_wait(self, slot: int, k=None) -> tuple:
        """Wait for the slot's read-back; returns (top-k records, trades of that run)."""
        k = k or self.topk
        out = np.zeros(k, TOPK_DTYPE)
        n = C.c_int64(0)
        m = _check(lib().bt_topk_fetch_wait(self._h, slot, out.ctypes.data, k, C.byref(n)))
        return out[:m], int(n.value)

    def replay(self, lanes, trade_cap: int = 0, curves: bool = False) -> Replay:
        """Replay chosen (symbol id, param) lanes of the resident dataset on the GPU
        (bt_replay): their full summaries, bar counts, the first trade_cap trades of each
        (trade_cap > 0) and, with curves, the equity curve E_t and position pos_t of every bar.
        `lanes`: top-k records (read_topk() feeds straight in), an (n, 2) integer array or a list
        of (sym, param) pairs; at most REPLAY_MAX per call. Rows come back in request order."""
        req = as_lanes(lanes)
        n = len(req)
        f = sym("bt_replay")
        summ = np.zeros(max(n, 1), SUMMARY_DTYPE)
        nb = np.zeros(max(n, 1), np.int32)
        tr = np.zeros((max(n, 1), trade_cap), TRADE_DTYPE) if trade_cap > 0 else None
        eq = ps = None
        stride = 0
        if curves:  # rows as long as the longest requested symbol
            stride = self._replay_stride(f, req) if 0 < n <= REPLAY_MAX else 1
            eq = np.empty((max(n, 1), stride), np.int64)
            ps = np.empty((max(n, 1), stride), np.int8)
        _check(f(self._h, n, req.ctypes.data if n else None, trade_cap, summ.ctypes.data,
                 nb.ctypes.data, _ptr(tr), _ptr(eq), _ptr(ps), stride))
        if curves:
            eq, ps = eq[:n], ps[:n]
            if n == 0:
                eq, ps = eq[:, :0], ps[:, :0]
        return Replay(req, summ[:n], nb[:n], None if tr is None else tr[:n], eq, ps)

    def _replay_stride(self, f, req) -> int:
        """Bars of the longest requested symbol. The bar counts of a dataset loaded through this
        object are known here; otherwise (run_batch) one replay without curves returns them."""
        bars = self._sym_bars
        if isinstance(bars, tuple):  # load_synthetic: ids begin .. begin + n, all of `bars` bars
            begin, n_sym, b = bars
            if ((req["sym"] >= begin) & (req["sym"] < begin + n_sym)).all():
                return b
        elif isinstance(bars, dict):
            got = [bars.get(int(s)) for s in np.unique(req["sym"])]
            if None not in got:
                return max(got)
        summ = np.zeros(len(req), SUMMARY_DTYPE)
        nb = np.zeros(len(req), np.int32)
        _check(f(self._h, len(req), req.ctypes.data, 0, summ.ctypes.data, nb.ctypes.data, None, None,
                 None, 0))
        return int(nb.max())

    # ---- reductions of the last run (bt_surface, k_surface.hip)
    def surface(self, best: bool = True) -> Surface:
        """The last run (run() or run_batch()) reduced on the GPU: one aggregate per parameter
        over every symbol and, with best, each symbol's best lane in dataset row order."""
        f = sym("bt_surface")
        S = self.stats()["n_symbols"]
        agg, rec = _surface_bufs(S, self.n_params, best)
        _check(f(self._h, agg.ctypes.data, _ptr(rec)))
        return Surface(agg[:self.n_params], None if rec is None else rec[:S])

    def surface_of(self, summaries, sym_ids, best: bool = True) -> Surface:
        """The same device kernels on a caller's S x P summary matrix (at most SURFACE_OF_MAX
        records) and its symbol ids."""
        m, ids = _as_matrix(summaries, sym_ids)
        S, P = m.shape
        agg, rec = _surface_bufs(S, P, best)
        _check(sym("bt_surface_of")(self._h, S, P, m.ctypes.data if m.size else None,
                                    ids.ctypes.data if S else None, agg.ctypes.data, _ptr(rec)))
        return Surface(agg[:P], None if rec is None else rec[:S])

    def topk_of(self, summaries, sym_ids, k: int, lds_free_hist: bool = False) -> np.ndarray:
        """The run's top-k chain (bt_topk_of, k_topk.hip) on a caller's S x P summary matrix (at
        most TOPK_OF_MAX records) and its symbol ids: the min(k, S*P) best records, as read_topk()
        returns them. lds_free_hist: the histogram kernel without LDS (up to 2^18 records)."""
        m, ids = _as_matrix(summaries, sym_ids)
        S, P = m.shape
        out = np.zeros(max(k, 1), TOPK_DTYPE)
        n = _check(sym("bt_topk_of")(self._h, S, P, m.ctypes.data if m.size else None,
                                     ids.ctypes.data if S else None, k, int(bool(lds_free_hist)),
                                     out.ctypes.data))
        return out[:n]

    def set_surface_chunks(self, n: int) -> None:
        """Symbol chunks surface() cuts the rows into: 0 = the planner's choice, n = always n
        (clipped to the symbol count). Results are identical either way."""
        _check(sym("bt_set_surface_chunks")(self._h, n))

    # ---- walk-forward evaluation (bt_walk_forward, k_walkfwd.hip)
    def walk_forward(self, bounds, train: int = 1, folds: bool = False) -> WalkForward:
        """Walk every (symbol, param) lane of the resident dataset once and cut its result into
        the bar folds [bounds[k], bounds[k+1]); per symbol and step j = max(train, 1) .. K-1
        choose the parameter with the best Sharpe over the `train` folds before fold j (all of
        them when train == 0) and report that lane's record of fold j. With folds, every lane's
        fold records come back too ([S, P, K], at most WALKFWD_FOLDS_MAX of them). run() need not
        have been called."""
        b = _as_bounds(bounds)
        K = len(b) - 1
        S = self.stats()["n_symbols"]
        n_steps = max(K - max(train, 1), 0)
        steps = np.zeros(max(S * n_steps, 1), WF_STEP_DTYPE)
        total = np.zeros(max(S, 1), FOLD_DTYPE)
        want = K >= 2  # a single fold has no step: only its records can be asked for
        rec = None
        if folds:
            if S * self.n_params * max(K, 0) > WALKFWD_FOLDS_MAX:
                raise BtError(f"bt_walk_forward: S*P*K = {S}*{self.n_params}*{K} exceeds 2^22 fold records")
            rec = np.zeros(max(S * self.n_params * max(K, 0), 1), FOLD_DTYPE)
        _check(sym("bt_walk_forward")(self._h, K, b.ctypes.data if len(b) else None, train, _ptr(rec),
                                      steps.ctypes.data if want else None, total.ctypes.data if want else None))
        return WalkForward(b, train, steps[:S * n_steps].reshape(S, n_steps), total[:S],
                           None if rec is None else rec[:S * self.n_params * K].reshape(S, self.n_params, K))

    def set_walkfwd_budget(self, nbytes: int) -> None:
        """Device staging budget of walk_forward in bytes: 0 = the default (256 MB). Results are
        identical whatever the budget."""
        _check(sym("bt_set_walkfwd_budget")(self._h, nbytes))

    # ---- probability of backtest overfitting (overfit.py, k_cscv.hip)
    def cscv(self, bounds=None, folds=None, sym_ids=None, hist: bool = True, picks: bool = False):
        """Combinatorially symmetric cross-validation (docs/cscv_spec.md): with `bounds` (K + 1 bar
        indices, K even in [2, CSCV_MAX_FOLDS]) every lane of the resident dataset is walked and cut
        into K folds as walk_forward cuts it, every symbol being one group of n_params lanes; with
        `folds` (FOLD_DTYPE[G, P, K], for example WalkForward.folds, and optionally sym_ids[G]) the
        same kernels run on those records. Per group, every way of taking K/2 folds as the in-sample
        half picks the lane with the best in-sample Sharpe and ranks it on the other half.
        Overfit.pbo() is the share of combinations whose pick ranks in the lower half there. With
        picks every combination's pick comes back (at most CSCV_PICKS_MAX records). The call, its
        records and its result type live in overfit.py."""
        from .overfit import engine_cscv
        return engine_cscv(self, bounds, folds, sym_ids, hist, picks)

    def set_cscv_work(self, cells: int) -> None:
        """The most (row, combination pair, lane) cells one launch of cscv covers: 0 = the default.
        Results are identical whatever the value."""
        _check(sym("bt_set_cscv_work")(self._h, cells))

    # ---- trade statistics and drawdown timing (bt_trade_stats, k_tstats.hip)
    def trade_stats(self, lanes=None, per_lane: bool = True, params: bool = False) -> TradeStats:
        """Per-lane trade statistics of the resident dataset (bt_trade_stats): wins and losses,
        gross profit and loss, streaks, holding times, the sum of squared trade pnl, and where the
        largest drawdown began and bottomed and how long the curve stayed under water. With
        `lanes` (what replay takes; at most TSTATS_MAX) the records of those lanes in request
        order; without, every lane as an [S, P] matrix (per_lane) and / or one aggregate per
        parameter over every symbol (params). With per_lane=False nothing of size S x P leaves the
        device. run() need not have been called."""
        f = sym("bt_trade_stats")
        if lanes is not None:
            if params:
                raise ValueError("trade_stats: params aggregates every lane of the dataset; leave lanes out")
            req = as_lanes(lanes)
            n = len(req)
            out = np.zeros(max(n, 1), TSTATS_DTYPE)
            keep = _list_mode(req)
            _check(f(self._h, n, keep.ctypes.data, out.ctypes.data, None))
            return TradeStats(out[:n], None)
        S, P = self.stats()["n_symbols"], self.n_params
        out = np.zeros(max(S * P, 1), TSTATS_DTYPE) if per_lane else None
        agg = np.zeros(max(P, 1), TSTATS_AGG_DTYPE) if params else None
        _check(f(self._h, 0, None, _ptr(out), _ptr(agg)))
        return TradeStats(None if out is None else out[:S * P].reshape(S, P), None if agg is None else agg[:P])

    def set_tstats_budget(self, nbytes: int) -> None:
        """Device staging budget of trade_stats in bytes: 0 = the default (256 MB). Results are
        identical whatever the budget."""
        _check(sym("bt_set_tstats_budget")(self._h, nbytes))

    # ---- net of costs (costs.py, k_costs.hip)
    def costs(self, levels, lanes=None, per_lane: bool = True, params: bool = False):
        """Every lane of the resident dataset under a ladder of fee levels (docs/costs_spec.md):
        `levels` is a sequence of at most 16 (fixed_ticks, bps) pairs, a fill at price px paying
        fixed_ticks + floor(px * bps / 10000). Per (lane, level): the net pnl, the fees, the net
        drawdown and where it bottoms, the bars under water, the sum of squared net increments and
        which trades still win. With `lanes` (what replay takes) the records of those lanes in
        request order, [n, C]; without, every lane as [S, P, C] (per_lane) and / or one aggregate
        per (parameter, level) over every symbol, [P, C] (params). With per_lane=False nothing of
        size S x P leaves the device. run() need not have been called. The call, its records and
        its result type live in costs.py."""
        from .costs import engine_costs
        return engine_costs(self, levels, lanes, per_lane, params)

    def set_costs_budget(self, nbytes: int) -> None:
        """Device staging budget of costs in bytes: 0 = the default (256 MB). Results are identical
        whatever the budget."""
        from .costs import engine_set_costs_budget
        engine_set_costs_budget(self, nbytes)

    # ---- tail risk (tail.py, k_tail.hip)
    def tail_risk(self, levels=(0.01, 0.05), lanes=None, window=None, held: bool = False):
        """The shape of every lane's per-bar pnl (docs/tail_spec.md): per lane the counts, the
        extremes and where they fall, and the exact power sums up to the fourth of its increments
        d_t over the window's bars (with `held` only the bars a position was held into), and per
        (lane, level) the value at risk and the expected shortfall as exact order statistics.
        `levels`: at most 8 lower-tail levels, fractions (0.05) or integer parts per million. With
        `lanes` (what replay takes) the records of those lanes in request order, [n]; without,
        every lane as [S, P]. run() need not have been called. The call, its records and its result
        type (TailRisk, with the moments, ratios, psr and deflated_sharpe) live in tail.py."""
        from .tail import engine_tail_risk
        return engine_tail_risk(self, levels, lanes, window, held)

    def tail_of(self, d, levels=(0.01, 0.05)):
        """The tail kernels on a caller's increments: an [n, T] integer array with |d| < 2^31. Every
        entry is counted. Needs no dataset."""
        from .tail import engine_tail_of
        return engine_tail_of(self, d, levels)

    def set_tail_row(self, mode: int) -> None:
        """Where tail_risk and tail_of keep a lane's row of counted increments: 0 = the planner's
        choice, 1 = LDS (refused at call time when the row does not fit), 2 = device memory.
        Results are identical under every setting."""
        from .tail import engine_set_tail_row
        engine_set_tail_row(self, mode)

    def set_tail_budget(self, nbytes: int) -> None:
        """Device staging budget of tail_risk and tail_of in bytes: 0 = the default (256 MB).
        Results are identical whatever the budget."""
        from .tail import engine_set_tail_budget
        engine_set_tail_budget(self, nbytes)

    def last_tail_row(self) -> int:
        """The row home the last tail_risk / tail_of used: 1 = LDS, 2 = device memory, 0 = none yet."""
        from .tail import engine_last_tail_row
        return engine_last_tail_row(self)

    # ---- bootstrap reality check (bt_bootstrap / bt_bootstrap_of, k_boot.hip)
    def reality_check(self, lanes=None, groups=None, resamples: int = 1000, block: int = 10, seed: int = 0,
                      window=None, per_lane: bool = False, vmax: bool = False, boot: bool = False) -> RealityCheck:
        """White's bootstrap reality check on the GPU (bt_bootstrap): is the best lane of a group
        luck? The per-bar pnl increments of all lanes over one window (by default every bar of the
        longest row) are resampled jointly, `resamples` times in circular blocks of `block` bars,
        and per group the best centred resampled sum is compared with the observed best sum.
        `lanes`: what replay takes (at most BOOT_MAX), with `groups` a list of group sizes (None:
        one group); without lanes every (symbol, param) lane of the resident dataset, one group per
        symbol. per_lane, vmax and boot ask for the lane records, the V* matrix and the raw
        resampled sums (boot with lanes only). run() need not have been called."""
        f = sym("bt_bootstrap")
        frm, to = (0, 0) if window is None else _window(window)
        B = int(resamples)
        Bb = B if 0 < B <= BOOT_MAX_RESAMPLES else 0   # a refused B sizes no buffer
        if lanes is None:
            if groups is not None:
                raise ValueError("reality_check: groups come with lanes; without lanes every symbol is a group")
            if boot:
                raise ValueError("reality_check: boot comes with lanes only")
            S, P = self.stats()["n_symbols"], self.n_params
            bufs = _boot_bufs(S * P, S, Bb, per_lane, vmax, False)
            _check(f(self._h, 0, None, 0, None, frm, to, B, int(block), _u64(seed), *(_ptr(b) for b in bufs)))
            return _boot_result(bufs, S * P, S, B)
        req = as_lanes(lanes)
        n = len(req)
        goff = _as_goff(groups, n)
        G = 1 if goff is None else len(goff) - 1
        bufs = _boot_bufs(n, G, Bb, per_lane, vmax, boot)
        keep = _list_mode(req)
        _check(f(self._h, n, keep.ctypes.data, G, _ptr(goff), frm, to, B, int(block), _u64(seed),
                 *(_ptr(b) for b in bufs)))
        return _boot_result(bufs, n, G, B)

    def bootstrap_of(self, d, groups=None, resamples: int = 1000, block: int = 10, seed: int = 0,
                     per_lane: bool = True, vmax: bool = True, boot: bool = False) -> RealityCheck:
        """The resampling and finish kernels (bt_bootstrap_of) on a caller's increments: an [n, T]
        integer array with |d| < 2^31, n at most BOOT_MAX. Needs no dataset."""
        a = _as_increments(d, "bootstrap_of")
        n, T = a.shape
        goff = _as_goff(groups, n)
        G = 1 if goff is None else len(goff) - 1
        B = int(resamples)
        bufs = _boot_bufs(n, G, B if 0 < B <= BOOT_MAX_RESAMPLES else 0, per_lane, vmax, boot)
        _check(sym("bt_bootstrap_of")(self._h, n, T, a.ctypes.data if a.size else None, G, _ptr(goff), B, int(block),
                                      _u64(seed), *(_ptr(b) for b in bufs)))
        return _boot_result(bufs, n, G, B)

    def set_boot_budget(self, nbytes: int) -> None:
        """Device staging budget of reality_check and bootstrap_of in bytes: 0 = the default
        (256 MB). Results are identical whatever the budget."""
        _check(sym("bt_set_boot_budget")(self._h, nbytes))

    def set_boot_row(self, mode: int) -> None:
        """Where a lane's prefix row lives while it is resampled: 0 = the planner's choice, 1 = LDS
        (refused at call time when the row does not fit), 2 = device memory. Results are identical
        either way."""
        _check(sym("bt_set_boot_row")(self._h, mode))

    # ---- drawdown bootstrap (ddrisk.py, k_ddboot.hip)
    def drawdown_risk(self, lanes=None, resamples: int = 1000, block: int = 10, seed: int = 0, window=None,
                      levels=(0.5, 0.95), limits=(), raw: bool = False):
        """How deep could each lane's drawdown be (docs/drawdown_spec.md)? The circular block
        bootstrap of reality_check (the same window, resamples, block and seed draw the same bars)
        of every lane's largest drawdown: per lane the observed drawdown, how many resampled paths
        reach it, the extremes and the exact sums of MDD* and MDD*^2, per level the quantile of
        MDD*, per limit how many paths draw down at least that far. `lanes`: what replay takes;
        without lanes every (symbol, param) lane of the resident dataset. `levels`: at most 8,
        fractions (0.95) or integer parts per million; `limits`: at most 8 losses in ticks; `raw`
        asks for the raw MDD* (with lanes only). run() need not have been called. The binding and
        the result type (DrawdownRisk) live in ddrisk.py."""
        from .ddrisk import engine_drawdown_risk
        return engine_drawdown_risk(self, lanes, resamples, block, seed, window, levels, limits, raw)

    def drawdown_of(self, d, resamples: int = 1000, block: int = 10, seed: int = 0, levels=(0.5, 0.95), limits=(),
                    raw: bool = False):
        """The drawdown kernels on a caller's increments: an [n, T] integer array with |d| < 2^31,
        n at most BOOT_MAX. Needs no dataset."""
        from .ddrisk import engine_drawdown_of
        return engine_drawdown_of(self, d, resamples, block, seed, levels, limits, raw)

    def set_ddboot_row(self, mode: int) -> None:
        """Where drawdown_risk and drawdown_of keep a lane's prefix row and block tables: 0 = the
        planner's choice, 1 = LDS (refused at call time when they do not fit), 2 = device memory.
        Results are identical either way."""
        from .ddrisk import engine_set_ddboot_row
        engine_set_ddboot_row(self, mode)

    def set_ddboot_budget(self, nbytes: int) -> None:
        """Device staging budget of drawdown_risk and drawdown_of in bytes: 0 = the default
        (256 MB). Results are identical whatever the budget."""
        from .ddrisk import engine_set_ddboot_budget
        engine_set_ddboot_budget(self, nbytes)

    def last_ddboot_row(self) -> int:
        """The row home the last drawdown_risk / drawdown_of used: 1 = LDS, 2 = device memory, 0 =
        none yet."""
        from .ddrisk import engine_last_ddboot_row
        return engine_last_ddboot_row(self)

    # ---- portfolio of chosen lanes (bt_portfolio, k_portfolio.hip)
    def portfolio(self, lanes, windows=None, n_bars=None) -> Portfolio:
        """Trade chosen (symbol id, param) lanes of the resident dataset together (bt_portfolio):
        per bar the book's pnl, equity and long / short counts, and one summary. `lanes`: what
        as_lanes accepts (top-k records, surface().best, pairs) with optional `windows` (one
        (from_bar, to_bar) pair or one per entry), or PF_LANE_DTYPE records such as
        walk_forward_lanes(wf); at most PORTFOLIO_MAX. Every entry is walked over its whole series
        and counts on its window only. `n_bars`: the bars of the result, by default those of the
        longest resident symbol (of the longest requested one after run_batch). run() need not have
        been called."""
        req = as_pf_lanes(lanes, windows)
        T = self._longest(req["sym"]) if n_bars is None else int(n_bars)
        bufs = _pf_bufs(T)
        _check(sym("bt_portfolio")(self._h, len(req), req.ctypes.data if len(req) else None, T,
                                   *(b.ctypes.data for b in bufs)))
        return _pf_result(bufs, T, self.grid.annualization)

    def _longest(self, syms) -> int:
        """Bars of the longest resident symbol when the dataset was loaded through this object,
        else (run_batch) of the longest of `syms`, asked from bt_replay REPLAY_MAX ids at a time."""
        bars = self._sym_bars
        if isinstance(bars, tuple):
            return bars[2]
        if isinstance(bars, dict) and bars:
            return max(bars.values())
        ids = np.unique(np.asarray(syms, np.int32))
        longest = 1
        for i in range(0, len(ids), REPLAY_MAX):
            part = np.zeros(len(ids[i:i + REPLAY_MAX]), LANE_DTYPE)
            part["sym"] = ids[i:i + REPLAY_MAX]
            longest = max(longest, self._replay_stride(sym("bt_replay"), part))
        return longest

    def set_portfolio_replicas(self, r: int) -> None:
        """Replicas of the per-bar accumulators portfolio() adds into: 0 = the planner's choice.
        Results are identical either way."""
        _check(sym("bt_set_portfolio_replicas")(self._h, r))

    # ---- covariance of chosen lanes (bt_covariance / bt_gram_of, k_gram.hip)
    def covariance(self, lanes, window=None) -> Covariance:
        """How chosen (symbol id, param) lanes of the resident dataset move together
        (bt_covariance): the exact Gram matrix and the sums of their per-bar pnl increments over
        one common window, by default every bar of the longest requested symbol. `lanes`: what
        replay takes (read_topk(), surface().best, pairs), at most COV_MAX. run() need not have
        been called."""
        req = as_lanes(lanes)
        n = len(req)
        frm, to = _window(window)
        wide, sums, T = np.zeros(max(n * n, 1), WIDE_DTYPE), np.zeros(max(n, 1), np.int64), C.c_int32(0)
        _check(sym("bt_covariance")(self._h, n, req.ctypes.data if n else None, frm, to, wide.ctypes.data,
                                    sums.ctypes.data, C.addressof(T)))
        return _cov_result(n, wide, sums, T.value)

    def gram_of(self, d) -> Covariance:
        """The Gram kernels (bt_gram_of) on a caller's increments: an [n, T] integer array with
        |d| < 2^31, n at most COV_MAX. Needs no dataset."""
        a = _as_increments(d, "gram_of")
        n, T = a.shape
        wide, sums = np.zeros(max(n * n, 1), WIDE_DTYPE), np.zeros(max(n, 1), np.int64)
        _check(sym("bt_gram_of")(self._h, n, T, a.ctypes.data if a.size else None, wide.ctypes.data,
                                 sums.ctypes.data))
        return _cov_result(n, wide, sums, T)

    def set_gram_split(self, k: int) -> None:
        """Bar chunks covariance() and gram_of() cut their window into: 0 = the planner's choice.
        Results are identical either way."""
        _check(sym("bt_set_gram_split")(self._h, k))

    def stats(self) -> dict:
        st = _Stats()
        _check(lib().bt_read_stats(self._h, C.byref(st)))
        return {f: getattr(st, f) for f, _ in _Stats._fields_}

    def close_column(self, sym_index, n) -> np.ndarray:
        out = np.zeros(n, np.int32)
        _check(lib().bt_read_close(self._h, sym_index, out.ctypes.data, n))
        return out

    def kernel_timing(self):
        ms, n, name = C.c_double(), C.c_int64(), C.c_char_p()
        _check(lib().bt_kernel_timing(self._h, C.byref(ms), C.byref(n), C.byref(name)))
        return ms.value, n.value, name.value.decode()

    def reset_timing(self):
        _check(lib().bt_reset_timing(self._h))

    # ---- the JobsReply batch (drop-in for process_incoming_job)
    def run_batch(self, jobs: Sequence[tuple]) -> list:
        """jobs: [(id: str, file: bytes)] -> [(status, data: str)] in job order."""
        n = len(jobs)
        jin = (_JobIn * max(n, 1))()
        keep = []
        for i, (jid, data) in enumerate(jobs):
            b = bytes(data)
            idb = jid.encode() if isinstance(jid, str) else bytes(jid)
            keep += [b, idb]
            jin[i].id = idb
            jin[i].file = C.cast(C.c_char_p(b), C.c_void_p)
            jin[i].len = len(b)
        jout = (_JobOut * max(n, 1))()
        self._sym_bars = None
        try:
            _check(lib().bt_run_batch(self._h, n, jin, jout))
            res = [(jout[i].status, C.string_at(jout[i].data, jout[i].len).decode()) for i in range(n)]
        finally:
            lib().bt_job_out_free(jout, n)  # safe on NULL entries, also after a failure
        return res

    def batch_profile(self) -> dict:
        """Phase times of the last run_batch (bt_last_batch_profile)."""
        pr = _BatchProfile()
        _check(lib().bt_last_batch_profile(self._h, C.byref(pr)))
        return {f: getattr(pr, f) for f, _ in _BatchProfile._fields_}


class Comm:
    """The multi-GPU exchange behind the C ABI (bt_comm_*, csrc/comm.cpp): one RCCL all-gather
    per run of every rank's top-k records and counters, from the engine's device buffers."""

    ID_BYTES = 128

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(Comm.ID_BYTES)
        _check(sym("bt_comm_unique_id")(buf))
        return buf.raw

    def __init__(self, uid: bytes, rank: int, world: int, device: int, k: int):
        if len(uid) != Comm.ID_BYTES:
            raise ValueError("RCCL unique id must be 128 bytes")
        err = C.create_string_buffer(512)
        self._uid = C.create_string_buffer(bytes(uid), Comm.ID_BYTES)
        h = sym("bt_comm_create")(self._uid, rank, world, device, k, err, 512)
        if not h:
            raise BtError(err.value.decode())
        self._h, self.k, self.world = h, k, world

    def exchange_async(self, engine: "Engine", slot: int) -> None:
        _check(sym("bt_exchange_async")(self._h, engine._h, slot))

    def exchange_wait(self, slot: int, k=None) -> tuple:
        """Merged global top-k and [bar-evals, trades] summed over ranks."""
        k = k or self.k
        out = np.zeros(k, TOPK_DTYPE)
        cnt = np.zeros(2, np.int64)
        m = _check(sym("bt_exchange_wait")(self._h, slot, out.ctypes.data, k, cnt.ctypes.data))
        return out[:m], [int(cnt[0]), int(cnt[1])]

    def close(self):
        if getattr(self, "_h", None):
            sym("bt_comm_destroy")(self._h)
            self._h = None

    __del__ = close


def merge_topk(records: np.ndarray, k: int) -> np.ndarray:
    """Host merge of shard top-k lists (same order as the device: sharpe desc, sym, param)."""
    recs = np.ascontiguousarray(records, TOPK_DTYPE)
    out = np.zeros(max(k, 1), TOPK_DTYPE)
    m = _check(lib().bt_merge_topk(recs.ctypes.data if len(recs) else None, len(recs), k,
                                   out.ctypes.data))
    return out[:m]


def exchange_message(records: np.ndarray, k_msg: int, bar_evals: int, trades: int) -> bytes:
    """One rank's exchange message as bt_exchange_async sends it (comm.cpp): a header record whose
    first int32 is the record count, k_msg record slots (the first n used), bar-evals, trades."""
    n = len(records)
    size = _check(sym("bt_exchange_message_bytes")(k_msg))
    buf = np.zeros(size, np.uint8)
    buf[:4] = np.frombuffer(np.int32(n).tobytes(), np.uint8)
    rec = TOPK_DTYPE.itemsize
    if n:
        buf[rec:rec * (1 + n)] = np.frombuffer(np.ascontiguousarray(records, TOPK_DTYPE).tobytes(), np.uint8)
    buf[rec * (k_msg + 1):] = np.frombuffer(np.array([bar_evals, trades], np.int64).tobytes(), np.uint8)
    return buf.tobytes()


def exchange_merge(block: bytes, world: int, k_msg: int, k: int) -> tuple:
    """The host half of Comm.exchange_wait (bt_exchange_merge) on a gathered block of `world`
    messages: the merged top-k and [bar-evals, trades] summed over ranks."""
    raw = np.frombuffer(block, np.uint8)
    need = world * _check(sym("bt_exchange_message_bytes")(k_msg))
    if len(raw) != need:  # the C side checks the same; fail before handing it a short buffer
        raise BtError(f"exchange block holds {len(raw)} bytes, expected {need} "
                      f"(world {world} x message of k_msg {k_msg})")
    out = np.zeros(max(k, 1), TOPK_DTYPE)
    cnt = np.zeros(2, np.int64)
    m = _check(sym("bt_exchange_merge")(raw.ctypes.data, len(raw), world, k_msg, out.ctypes.data,
                                        k, cnt.ctypes.data))
    return out[:m], [int(cnt[0]), int(cnt[1])]


def format_summaries(rows: np.ndarray) -> str:
    """The CompleteRequest.data text bt_run_batch writes for these summaries (spec §6)."""
    rows = np.ascontiguousarray(rows, SUMMARY_DTYPE)
    cap = _check(lib().bt_format_summaries(None, len(rows), None, 0))
    buf = C.create_string_buffer(max(cap, 1))
    n = _check(lib().bt_format_summaries(rows.ctypes.data if len(rows) else None, len(rows), buf, cap))
    return buf.raw[:n].decode()


def i128_to_double(lo: int, hi: int) -> float:
    return lib().bt_i128_to_double(lo & ((1 << 64) - 1), hi)


def parse_csv(data: bytes, cap=1 << 22):
    """Host ingest of one Job.File (CSV or binary columns) -> (high, low, close) int32 ticks."""
    cap = int(cap)
    h, lo, c = (np.empty(cap, np.int32) for _ in range(3))
    err = C.create_string_buffer(256)
    n = lib().bt_parse_job(data, len(data), cap, h.ctypes.data, lo.ctypes.data, c.ctypes.data,
                           err, 256)
    if n < 0:
        raise ValueError(err.value.decode())
    return h[:n].copy(), lo[:n].copy(), c[:n].copy()
