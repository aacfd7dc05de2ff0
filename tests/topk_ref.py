"""The top-k of an S x P summary matrix by a plain sort, written from the order of bt_topk_rec
(include/bt.h) alone: Sharpe descending by its orderable bit pattern, then symbol id ascending as
a signed int32, then param ascending. The reference of tests/test_gpu_topk_keys.py and
tests/test_topk_cases_cpu.py; it shares nothing with the package but the two record dtypes."""
import numpy as np

import dbx_amd as D

TOP = np.uint64(1 << 63)


def order_key(sharpe) -> np.ndarray:
    """The order key of doubles as uint64, monotone in the order of the Sharpe: a set sign bit
    complements the word, a clear one sets the top bit (+0.0 lands above -0.0)."""
    u = np.ascontiguousarray(sharpe, np.float64).view(np.uint64)
    return np.where(u >> np.uint64(63) != 0, ~u, u | TOP)


def topk(summaries, sym_ids, k: int) -> np.ndarray:
    """The first min(k, S*P) records of the matrix in the order above, as TOPK_DTYPE: the Sharpe's
    bits, the row's id, the param and the pnl of each."""
    m = np.asarray(summaries)
    S, P = m.shape
    flat = m.reshape(-1)
    key = order_key(flat["sharpe"])
    sym = np.repeat(np.asarray(sym_ids).astype(np.int32), P)
    param = np.tile(np.arange(P, dtype=np.int32), S)
    idx = np.lexsort((param, sym, ~key))[:min(k, S * P)]   # last key first: ~key ascending = key descending
    out = np.zeros(len(idx), D.TOPK_DTYPE)
    out["sharpe"].view(np.uint64)[:] = flat["sharpe"][idx].view(np.uint64)
    out["sym"], out["param"], out["pnl"] = sym[idx], param[idx], flat["pnl"][idx]
    return out


def topk_brute(summaries, sym_ids, k: int) -> list:
    """The same by sorted() over Python tuples (small cases): (sharpe bits, sym, param, pnl)."""
    m = np.asarray(summaries)
    S, P = m.shape
    rows = []
    for s in range(S):
        for p in range(P):
            bits = int(m[s, p]["sharpe"].view(np.uint64))
            key = (~bits & (2**64 - 1)) if bits >> 63 else bits | (1 << 63)
            rows.append((-key, int(np.int32(sym_ids[s])), p, bits, int(m[s, p]["pnl"])))
    return [(b, s, p, pnl) for _, s, p, b, pnl in sorted(rows)[:min(k, S * P)]]


def as_tuples(recs) -> list:
    r = np.asarray(recs, D.TOPK_DTYPE)
    return list(zip(r["sharpe"].view(np.uint64).tolist(), r["sym"].tolist(), r["param"].tolist(), r["pnl"].tolist()))
