"""Reference for the surface tests (tests only): docs/surface_spec.md restated in plain Python over
an S x P matrix of summaries. Sums are Python ints, so the 128-bit values are exact; orderings use
the engine's order key rebuilt with struct from the double's bits. Imports nothing from the
library: the record layouts below are written out again on purpose."""
import struct

import numpy as np

SUMMARY = np.dtype([("n_trades", "<i4"), ("status", "<i4"), ("pnl", "<i8"), ("mdd", "<i8"),
                    ("exposure", "<i8"), ("sharpe", "<f8"), ("hash", "<u8")])
PARAM_AGG = np.dtype([("n_sym", "<i4"), ("n_traded", "<i4"), ("n_win", "<i4"), ("n_pos", "<i4"),
                      ("trades", "<i8"), ("pnl", "<i8"), ("exposure", "<i8"), ("mdd_max", "<i8"),
                      ("sharpe_max", "<f8"), ("sharpe_min", "<f8"), ("sym_max", "<i4"), ("sym_min", "<i4"),
                      ("ss1_lo", "<u8"), ("ss1_hi", "<i8"), ("ss2_lo", "<u8"), ("ss2_hi", "<i8")])
TOPK = np.dtype([("sharpe", "<f8"), ("sym", "<i4"), ("param", "<i4"), ("pnl", "<i8")])
M64 = (1 << 64) - 1


def order_key(x) -> int:
    """The double's bits as an unsigned integer that orders like the value (-0.0 below +0.0)."""
    u = struct.unpack("<Q", struct.pack("<d", float(x)))[0]
    return (~u & M64) if u >> 63 else (u | (1 << 63))


def qs(sharpe) -> int:
    """clamp(sharpe, +-2^15) * 2^32, rounded half to even: the product is exact in double and
    float.as_integer_ratio gives it as an exact fraction."""
    x = float(sharpe)
    if x != x:
        return 0
    x = min(max(x, -32768.0), 32768.0)
    num, den = (x * 4294967296.0).as_integer_ratio()
    q, r = divmod(num, den)        # floor and remainder, 0 <= r < den
    if 2 * r > den or (2 * r == den and q & 1):
        q += 1
    return q


def _words(v: int):
    """A Python int as (lo uint64, hi int64) of its 128-bit two's complement."""
    assert -(1 << 127) <= v < (1 << 127)
    u = v & ((1 << 128) - 1)
    hi = u >> 64
    return u & M64, hi - (1 << 64) if hi >> 63 else hi


def aggregate(rows, ids):
    """One PARAM_AGG record from a column's summaries, given as tuples in SUMMARY field order
    (ndarray.tolist(): Python ints and floats, the doubles bit for bit), and their symbol ids."""
    out = np.zeros((), PARAM_AGG)
    out["sym_max"] = out["sym_min"] = -1
    n = traded = win = pos = trades = pnl = expo = ss1 = ss2 = 0
    mdd = None
    kmax = kmin = None   # (key, id, sharpe)
    for (r_trades, r_status, r_pnl, r_mdd, r_expo, sh, _hash), i in zip(rows, ids):
        if r_status != 0:
            continue
        n += 1
        traded += r_trades > 0
        win += r_pnl > 0
        pos += sh > 0
        trades += r_trades
        pnl += r_pnl
        expo += r_expo
        mdd = r_mdd if mdd is None else max(mdd, r_mdd)
        q = qs(sh)
        ss1 += q
        ss2 += q * q
        k = order_key(sh)
        if kmax is None or k > kmax[0] or (k == kmax[0] and i < kmax[1]):
            kmax = (k, i, sh)
        if kmin is None or k < kmin[0] or (k == kmin[0] and i < kmin[1]):
            kmin = (k, i, sh)
    out["n_sym"], out["n_traded"], out["n_win"], out["n_pos"] = n, traded, win, pos
    out["trades"], out["pnl"], out["exposure"] = trades, pnl, expo
    if n:
        out["mdd_max"] = mdd
        out["sharpe_max"], out["sym_max"] = kmax[2], kmax[1]
        out["sharpe_min"], out["sym_min"] = kmin[2], kmin[1]
    out["ss1_lo"], out["ss1_hi"] = _words(ss1)
    out["ss2_lo"], out["ss2_hi"] = _words(ss2)
    return out


def _matrix(summaries):
    m = np.asarray(summaries)
    assert m.ndim == 2 and m.dtype.itemsize == SUMMARY.itemsize
    return m.view(SUMMARY) if m.dtype != SUMMARY else m


def surface_ref(summaries, sym_ids):
    """(params PARAM_AGG[P], best TOPK[S]) of an S x P summary matrix and its S symbol ids."""
    m = _matrix(summaries)
    S, P = m.shape
    ids = [int(i) for i in sym_ids]
    assert len(ids) == S
    rows = m.tolist()
    params = np.zeros(P, PARAM_AGG)
    for p in range(P):
        params[p] = aggregate([row[p] for row in rows], ids)
    best = np.zeros(S, TOPK)
    for s, row in enumerate(rows):
        keys = [order_key(r[5]) for r in row]
        p = max(range(P), key=lambda j: (keys[j], -j))   # Sharpe descending, then param ascending
        best[s] = (row[p][5], ids[s], p, row[p][2])
    return params, best


def ties(summaries, sym_ids):
    """How often each tie rule decides: columns whose largest / smallest key occurs in more than
    one counted row, and rows whose best key occurs in more than one lane."""
    m = _matrix(summaries)
    n_max = n_min = n_best = 0
    for p in range(m.shape[1]):
        k = [order_key(r["sharpe"]) for r in m[:, p] if int(r["status"]) == 0]
        if k:
            n_max += k.count(max(k)) > 1
            n_min += k.count(min(k)) > 1
    for s in range(m.shape[0]):
        k = [order_key(x) for x in m[s]["sharpe"]]
        n_best += k.count(max(k)) > 1
    return n_max, n_min, n_best
