"""Crafted key sets for the top-k chain (k_topk.hip), one per path of the radix select, at the
smallest sizes that still reach the path. Every Sharpe is built from a bit pattern; `pnl` tags a
record with its flat index (records equal in key, id and param, which only repeated ids give, share
one tag, so the expected bytes are unique). NaN patterns are left out: sharpe_fx (internal.h)
produces none, and their place in the order is nobody's contract.

Each builder states in `want` what the device must meet on its case; path_counts() computes the
same figures from the records with a small restatement of the select's digit counting, and
tests/test_topk_cases_cpu.py asserts that they agree, so a case that does not reach its path fails
without a GPU.

Sizes that follow from the contents, not the other way round: `low_bits` holds 6,000 records of
which 5,000 share the prefix, so at k = 1,024 it cannot have k - 1 records above the group: 37 lie
above it, as at k = 100 (k = 1 has none). `signs` carries 2,100 records of -0.0 beside the others
and is 120 x 25; `signs_neg` (40 x 25) adds the cut inside the proper negatives, which k <= 1,024
cannot reach past that many zeros."""
import functools
from dataclasses import dataclass, field

import numpy as np

import dbx_amd as D
from topk_ref import order_key

CAP = 2048            # kTopkCap: records the finish block sorts in LDS
U = np.uint64


@dataclass
class Case:
    name: str
    summaries: np.ndarray      # SUMMARY_DTYPE[S, P]
    ids: np.ndarray            # int32[S]
    k: int
    want: dict = field(default_factory=dict)

    @property
    def n(self):
        return self.summaries.size


def bits_of_key(key) -> np.ndarray:
    """The double (as bits) whose order key is `key`: the inverse of topk_ref.order_key."""
    key = np.asarray(key, U)
    return np.where(key >> U(63) != 0, key & ~U(1 << 63), ~key)


def key_of(x: float) -> int:
    return int(order_key(np.array([x]))[0])


def _case(name, S, P, keys, ids, k, want):
    """keys: the flat uint64 order keys, record i = (row i // P, param i % P)."""
    keys = np.asarray(keys, U)
    assert keys.shape == (S * P,) and len(ids) == S
    bits = bits_of_key(keys)
    assert not np.isnan(bits.view(np.float64)).any(), name
    ids = np.asarray(ids, np.int64)
    assert ids.min() >= 0 and ids.max() < 2**31
    m = np.zeros(S * P, D.SUMMARY_DTYPE)
    m["sharpe"].view(U)[:] = bits
    m["pnl"] = np.arange(S * P)
    m["n_trades"] = 1 + np.arange(S * P) % 7
    m["hash"] = np.arange(S * P, dtype=U) * U(0x9E3779B97F4A7C15)
    if len(np.unique(ids)) < S:   # equal (key, id, param): one tag, the lowest flat index
        sym = np.repeat(ids, P)
        par = np.tile(np.arange(P), S)
        order = np.lexsort((np.arange(S * P), par, sym, keys))
        ks, ss, ps = keys[order], sym[order], par[order]
        first = np.ones(S * P, bool)
        first[1:] = (ks[1:] != ks[:-1]) | (ss[1:] != ss[:-1]) | (ps[1:] != ps[:-1])
        head = np.maximum.accumulate(np.where(first, np.arange(S * P), 0))   # the group's first position
        m["pnl"][order] = order[head]
    return Case(name, m.reshape(S, P), ids.astype(np.int32), k, want)


# ------------------------------------------------------------------ the select's digit counting
def _pick(digits, width, need):
    """The bin holding the need-th record counted from the top bin, the records above it and the
    non-empty bins (the last bin and the total when there are fewer records than need)."""
    h = np.bincount(digits.astype(np.int64), minlength=1 << width)[::-1]   # from the top
    cum = np.cumsum(h)
    j = int(np.searchsorted(cum, need)) if cum[-1] >= need else (1 << width) - 1
    return (1 << width) - 1 - j, int(cum[j] - h[j]), int((h > 0).sum())


def path_counts(summaries, ids, k) -> dict:
    """What the chain meets on these records: the selected 24-bit prefix, the records above it and
    sharing it, whether the finish takes the tie path, and on that path per later digit (key28,
    key16, key4, key0, then tb52 .. tb4, tb0 of the complemented (id, param) word) the non-empty
    bins and the records above the chosen one."""
    S, P = summaries.shape
    key = order_key(summaries.reshape(-1)["sharpe"])
    need = min(k, S * P)
    d1, a1, _ = _pick(key >> U(52), 12, need)
    in1 = key >> U(52) == U(d1)
    d2, a2, _ = _pick((key[in1] >> U(40)) & U(0xFFF), 12, need - a1)
    prefix = (d1 << 12) | d2
    top = key >> U(40)
    out = {"prefix24": prefix, "n_above": int((top > U(prefix)).sum()), "n_cand": int((top == U(prefix)).sum()),
           "need_group": need - a1 - a2}
    out["ties"] = out["n_above"] + out["n_cand"] > CAP
    if not out["ties"]:
        return out
    passes = []
    need = out["need_group"]
    sel = key[top == U(prefix)]
    pre = prefix << 40
    for shift, width in ((28, 12), (16, 12), (4, 12), (0, 4)):
        b, above, bins = _pick((sel >> U(shift)) & U((1 << width) - 1), width, need)
        passes.append((f"key{shift}", bins, above))
        need -= above
        pre |= b << shift
        sel = sel[(sel >> U(shift)) & U((1 << width) - 1) == U(b)]
    eq = np.flatnonzero(key == U(pre))
    word = (np.asarray(ids).astype(np.int64).astype(U)[eq // P] << U(32)) | (eq % P).astype(U)
    c = ~word
    for shift, width in ((52, 12), (40, 12), (28, 12), (16, 12), (4, 12), (0, 4)):
        b, above, bins = _pick((c >> U(shift)) & U((1 << width) - 1), width, need)
        passes.append((f"tb{shift}", bins, above))
        need -= above
        c = c[(c >> U(shift)) & U((1 << width) - 1) == U(b)]
    out.update(key=pre, passes=passes, need_equal=need, n_equal=len(c),
               nontrivial=[n for n, bins, _ in passes if bins > 1],
               above_nonzero=[n for n, _, above in passes if above > 0])
    return out


# ------------------------------------------------------------------------------------ builders
def _rand_keys(rng, n, lo24, hi24):
    """n keys with a 24-bit prefix in [lo24, hi24) and random low 40 bits."""
    return (rng.integers(lo24, hi24, n).astype(U) << U(40)) | rng.integers(0, 1 << 40, n).astype(U)


def _distinct_keys(rng, n, lo24, hi24):
    k = np.unique(_rand_keys(rng, 2 * n + 16, lo24, hi24))
    assert len(k) >= n
    return rng.permutation(k)[:n]


SEL = 0xC05123          # a prefix among the ordinary positive doubles (about 70)
POS_TOP = 0xFFE000      # below the infinities and NaNs
NEG_BOT = 0x001000      # above -inf and the negative NaNs


def boundary(shared: int) -> Case:
    """61 x 50, k = 1,024: 1,000 distinct records above the selected prefix, `shared` records with
    it, fillers below. 1,048: n_above + n_cand == 2,048, the LDS sort at m == cap; 1,049: the tie
    path by one record."""
    rng = np.random.default_rng(shared)
    S, P = 61, 50
    keys = np.concatenate([_distinct_keys(rng, 1000, SEL + 1, POS_TOP),
                           (U(SEL) << U(40)) | rng.permutation(1 << 20)[:shared].astype(U) * U(0x10001),
                           _rand_keys(rng, S * P - 1000 - shared, NEG_BOT, SEL)])
    name = "sort_full" if shared == 1048 else "tie_first"
    want = {"prefix24": SEL, "n_above": 1000, "n_cand": shared, "ties": shared + 1000 > CAP, "need_group": 24}
    return _case(name, S, P, rng.permutation(keys), 100 + rng.permutation(S), 1024, want)


def _tree_low40(rng, n, fan=5):
    """Low 40 key bits drawn level by level from `fan` values per 12-bit digit, the larger values
    the rarer, and all 16 last digits: every pass of the tie finish meets several bins, and a cut a
    few dozen or a few hundred records into the group has passed whole bins at every level."""
    w = (0.005, 0.1, 0.3, 0.3, 0.295)
    lv = [np.sort(rng.choice(1 << 12, fan, replace=False))[::-1].astype(U) for _ in range(3)]
    pick = lambda v: v[rng.choice(fan, n, p=w)]
    return (pick(lv[0]) << U(28)) | (pick(lv[1]) << U(16)) | (pick(lv[2]) << U(4)) | rng.integers(0, 16, n).astype(U)


def low_bits(k: int) -> Case:
    """120 x 50: 5,000 records share one 24-bit prefix and differ in the low 40 bits; 0 (k = 1) or
    37 (k = 100, k = 1,024) records lie above it and the cut falls inside the group."""
    rng = np.random.default_rng(7)
    S, P = 120, 50
    above = {1: 0, 100: 37, 1024: 37}[k]
    keys = np.concatenate([_distinct_keys(rng, above, SEL + 1, POS_TOP),
                           (U(SEL) << U(40)) | _tree_low40(rng, 5000),
                           _rand_keys(rng, S * P - 5000 - above, NEG_BOT, SEL)])
    want = {"prefix24": SEL, "n_above": above, "n_cand": 5000, "ties": True, "need_group": k - above}
    if k > 1:   # every low-bit pass: several bins, and records above the chosen one
        want.update(nontrivial=["key28", "key16", "key4", "key0"], above_nonzero=["key28", "key16", "key4", "key0"])
    return _case(f"low_bits_k{k}", S, P, rng.permutation(keys), rng.permutation(S) * 3 + 11, k, want)


def last_digit() -> Case:
    """120 x 50, k = 1,000: 5,000 records differ only in key bits 3..0 (312 or 313 per value), 100
    lie above. 900 are wanted from the group: values 15 and 14 whole and 276 of value 13, so the
    4-bit pass and the (sym, param) phase both decide."""
    rng = np.random.default_rng(11)
    S, P = 120, 50
    base = (U(SEL) << U(40)) | U(0x5A5A5A5A50)
    keys = np.concatenate([_distinct_keys(rng, 100, SEL + 1, POS_TOP), base | (np.arange(5000) % 16).astype(U),
                           _rand_keys(rng, S * P - 5100, NEG_BOT, SEL)])
    want = {"prefix24": SEL, "n_above": 100, "n_cand": 5000, "ties": True, "need_group": 900,
            "key": int(base) | 13, "need_equal": 1, "nontrivial": ["key0", "tb40", "tb4", "tb0"], "above_nonzero": ["key0", "tb40"]}
    return _case("last_digit", S, P, rng.permutation(keys), rng.permutation(S) * 1001 + 5, 1000, want)


ONE_KEY = 0xBFF8123456789ABC   # one ordinary positive double with no zero digit


def id_digits(repeat: bool = False) -> Case:
    """96 x 64, k = 1,024: about 6,000 records of one key, the others above it, so the whole cut is
    the (id, param) phase. The 13 lowest ids take 832 records whole; the cut falls in the row of id
    0x12355, whose neighbours 0x12340 and 0x123FF share its id bits 31..8: the 52-, 40- and 28-bit
    digits of the complement each meet several bins. `repeat`: three rows carry id 0x12355 and the
    cut falls inside one of their triples of equal records (need_equal 1 of 3)."""
    rng = np.random.default_rng(13 + repeat)
    S, P = 96, 64
    low = [0, 1, 9, 77, 200, 255, 1 << 8, 300, 1000, (1 << 12) - 1, (1 << 12) + 1, 5000, 0x12340]
    cut = [0x12355] * (3 if repeat else 1)
    high = [0x123FF, 1 << 20, (1 << 20) + 1, (1 << 24) + 5, 2**31 - 1]
    rest = S - len(low) - len(cut) - len(high)
    others = np.unique(rng.integers(1 << 20, 2**31 - 1, 4 * rest))
    others = rng.permutation(np.setdiff1d(others, high))[:rest]
    ids = rng.permutation(np.array(low + cut + high + others.tolist(), np.int64))   # unsorted rows
    n_above = 143 if repeat else 144
    keys = np.full(S * P, ONE_KEY, U)
    big = np.flatnonzero(np.repeat(ids, P) >= 1 << 20)       # the rows the cut never reaches
    keys[rng.permutation(big)[:n_above]] = _distinct_keys(rng, n_above, (ONE_KEY >> 40) + 1, POS_TOP)
    want = {"prefix24": ONE_KEY >> 40, "n_above": n_above, "n_cand": S * P - n_above, "ties": True,
            "need_group": 1024 - n_above, "key": ONE_KEY, "nontrivial": ["tb52", "tb40", "tb28", "tb4", "tb0"],
            "above_nonzero": ["tb40", "tb28"], "need_equal": 1, "n_equal": 3 if repeat else 1}
    return _case("repeated_ids" if repeat else "id_digits", S, P, keys, ids, 1024, want)


def _sign_values(rng, n_pos, n_pzero, n_nzero, n_neg):
    """Sharpe bit patterns by sign class: n_pos distinct positives above +0.0 with +inf (twice), the
    largest finite, 1e-300 and denormals among them; zeros; n_neg negatives with their mirror
    images, -inf twice."""
    f = lambda x: np.array(x, np.float64).view(U)
    special = f([np.inf, np.inf, 1.7976931348623157e308, 1e-300, 5e-324, 1e-310, 2.5e-320])
    ordinary = np.unique(np.abs(rng.normal(0, 3, 2 * (n_pos + n_neg))))
    ordinary = rng.permutation(ordinary[ordinary > 1e-3])
    pos = np.concatenate([special, f(ordinary[:n_pos - len(special)])])
    neg = np.concatenate([special, f(ordinary[n_pos:n_pos + n_neg - len(special)])]) | U(1 << 63)
    assert len(pos) == n_pos and len(neg) == n_neg
    return np.concatenate([pos, np.zeros(n_pzero, U), np.full(n_nzero, 1 << 63, U), neg])


def signs(k: int) -> Case:
    """120 x 25: 450 positives (+inf, the largest finite, 1e-300, denormals, ordinary), 150 of
    +0.0, 2,100 of -0.0 and 300 negatives (the mirror images, -inf). k = 10 cuts in the positives,
    k = 600 exactly between +0.0 and -0.0, k = 1,000 inside the records of -0.0: the tie path on
    the key 0x7FFF...F, with the negative denormals in its prefix group."""
    rng = np.random.default_rng(17)
    S, P = 120, 25
    bits = rng.permutation(_sign_values(rng, 450, 150, 2100, 300))
    keys = order_key(bits.view(np.float64))
    want = {10: {"ties": False},
            # the prefix group of a zero holds the denormals below 2^40 units too: 5e-324 and 2.5e-320
            600: {"prefix24": 0x800000, "n_above": 448, "n_cand": 152, "ties": False, "need_group": 152},
            1000: {"prefix24": 0x7FFFFF, "n_above": 600, "n_cand": 2102, "ties": True, "need_group": 400,
                   "key": 2**63 - 1, "need_equal": 1, "nontrivial": ["key4", "key0", "tb40", "tb0"]}}[k]
    return _case(f"signs_k{k}", S, P, keys, rng.permutation(S) * 7919 + 2, k, want)


def signs_neg() -> Case:
    """40 x 25, k = 600: 300 positives, 50 of each zero, 600 negatives: the cut falls inside the
    proper negatives, whose keys are the complemented words."""
    rng = np.random.default_rng(19)
    S, P = 40, 25
    bits = rng.permutation(_sign_values(rng, 300, 50, 50, 600))
    keys = order_key(bits.view(np.float64))
    return _case("signs_neg", S, P, keys, rng.permutation(S) + 1, 600, {"ties": False})


def short(S: int, P: int, k: int) -> Case:
    """n < k, k == n and a single record."""
    rng = np.random.default_rng(100 * S + 10 * P + k)
    keys = order_key(rng.normal(0, 1, S * P))
    return _case(f"short_{S}x{P}_k{k}", S, P, keys, rng.permutation(S) + 40, k, {"ties": False})


def blocks() -> Case:
    """250 x 80 = 20,000 records of N(0, 3), k = 100: three histogram blocks, the sort path."""
    rng = np.random.default_rng(23)
    S, P = 250, 80
    return _case("blocks", S, P, order_key(rng.normal(0, 3, S * P)), rng.permutation(S) + 1000, 100, {"ties": False})


STRIDE_ROWS, STRIDE_P = 33, 70_001
TIED = key_of(2.5)


def stride() -> Case:
    """33 x 70,001 = 2,310,033 records, k = 1,024: past 256 blocks x 8,192 records, so the
    histogram and collect kernels make a second grid-stride iteration, and P > 2^16, so the param
    digits of the complement at shifts 16 and 4 meet several bins. 500 distinct records lie above
    3,000 records tied at 2.5, the others (N(0, 0.4), below 2) under them. 400 of the tied lie in
    the row of the lowest id and 400 in the next, so the 524 wanted end inside that row."""
    rng = np.random.default_rng(29)
    S, P = STRIDE_ROWS, STRIDE_P
    x = np.minimum(rng.normal(0, 0.4, S * P), 1.9375)
    ids = rng.permutation(np.unique(rng.integers(0, 2**31, 2 * S))[:S])
    by_id = np.argsort(ids)
    where = rng.permutation(S * P)
    r0, r1 = (np.arange(P) + int(r) * P for r in by_id[:2])
    tied = np.concatenate([rng.permutation(r0)[:400], rng.permutation(r1)[:400]])
    others = where[~np.isin(where // P, by_id[:2])]
    tied = np.concatenate([tied, others[:2200]])
    keys = order_key(x)
    keys[tied] = TIED
    keys[others[2200:2700]] = _distinct_keys(rng, 500, (TIED >> 40) + 0x400, POS_TOP)
    want = {"prefix24": TIED >> 40, "n_above": 500, "n_cand": 3000, "ties": True, "need_group": 524, "key": TIED,
            "need_equal": 1, "n_equal": 1, "nontrivial": ["tb52", "tb16", "tb4"], "above_nonzero": ["tb52", "tb4"]}
    return _case("stride", S, P, keys, ids, 1024, want)


BUILDERS = {
    "sort_full": lambda: boundary(1048),
    "tie_first": lambda: boundary(1049),
    "low_bits_k1": lambda: low_bits(1),
    "low_bits_k100": lambda: low_bits(100),
    "low_bits_k1024": lambda: low_bits(1024),
    "last_digit": last_digit,
    "id_digits": id_digits,
    "repeated_ids": lambda: id_digits(True),
    "signs_k10": lambda: signs(10),
    "signs_k600": lambda: signs(600),
    "signs_k1000": lambda: signs(1000),
    "signs_neg": signs_neg,
    **{f"short_{S}x{P}_k{k}": (lambda S=S, P=P, k=k: short(S, P, k))
       for S, P in ((1, 1), (1, 7), (7, 1)) for k in (1, 7, 50)},
    "blocks": blocks,
    "stride": stride,
}
SMALL = [n for n in BUILDERS if n != "stride"]          # S*P <= 2^18: both histogram kernels


@functools.lru_cache(None)
def case(name: str) -> Case:
    """The case, built once per session; its arrays are read-only."""
    c = BUILDERS[name]()
    assert c.name == name
    c.summaries.setflags(write=False)
    c.ids.setflags(write=False)
    return c


# ------------------------------------------------------------------- shards and the host merges
def shards(c: Case, world: int = 3) -> list:
    """The case's rows as `world` contiguous shards: [(summaries, ids)]."""
    cut = [c.summaries.shape[0] * r // world for r in range(world + 1)]
    return [(c.summaries[a:b], c.ids[a:b]) for a, b in zip(cut[:-1], cut[1:])]


class Loopback:
    """torch.distributed as dbx_amd.parallel uses it, for `world` ranks played one after the other
    in one process: while recording, a collective keeps what the rank sends (and hands it its own
    message back from every rank); replaying, it delivers what every rank sent."""

    def __init__(self, world):
        self.world, self.rank, self.replay, self.call = world, 0, False, 0
        self.sent = [[] for _ in range(world)]

    def get_world_size(self):
        return self.world

    def get_backend(self):
        return "gloo"

    def _from(self, r, t):
        if not self.replay:
            return t
        return self.sent[r][self.call]

    def _done(self, t):
        if self.replay:
            self.call += 1
        else:
            self.sent[self.rank].append(t.clone())

    def all_gather(self, outs, t):
        for r, o in enumerate(outs):
            o.copy_(self._from(r, t))
        self._done(t)

    def all_gather_into_tensor(self, out, t):
        import torch
        out.copy_(torch.cat([self._from(r, t) for r in range(self.world)]))
        self._done(t)


def played(parts, fn):
    """fn(local records, dist) of dbx_amd.parallel as rank 0 of len(parts) ranks holding `parts`."""
    dist = Loopback(len(parts))
    for dist.rank, p in enumerate(parts):
        fn(p, dist)
    dist.replay = True
    return fn(parts[0], dist)
