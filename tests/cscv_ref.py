"""Reference for the CSCV tests (tests only), written from docs/cscv_spec.md alone: Python ints for
every sum, the oracle's Sharpe (oracle_np._sharpe), the engine's order (walkfwd_ref.key) and
itertools.combinations sorted by mask for the combination order. It shares nothing with cscv.cpp or
the kernel: both halves are summed on their own and ranks are counted by plain loops."""
import functools
import itertools

import numpy as np

import dbx_amd as D
import oracle_np as N
from walkfwd_ref import _join, key, n_ret


@functools.lru_cache(None)
def masks(K):
    """The C = binom(K, K/2) masks in combination order (bit k = fold k in-sample)."""
    return tuple(sorted(sum(1 << k for k in c) for c in itertools.combinations(range(K), K // 2)))


def ref_group(f, ann):
    """One group's (counts dict, hist list[2P - 1], picks list[C] of (lane, r2, is, oos), equals
    list[C]: the lanes level with each pick out of sample) from its fold records f[P, K]."""
    P, K = f.shape
    nret = [n_ret(int(f[0, k]["first_bar"]), int(f[0, k]["n_bars"])) for k in range(K)]
    s1 = [[_join(f[p, k]["s1_lo"], f[p, k]["s1_hi"]) for k in range(K)] for p in range(P)]
    s2 = [[_join(f[p, k]["s2_lo"], f[p, k]["s2_hi"]) for k in range(K)] for p in range(P)]
    cnt = dict(n_live=0, n_dead=0, n_overfit=0, n_loss=0, n_tied=0)
    hist = [0] * (2 * P - 1)
    picks, equals = [], []
    for m in masks(K):
        ins = [k for k in range(K) if m >> k & 1]
        oos = [k for k in range(K) if not m >> k & 1]
        n_is, n_oos = sum(nret[k] for k in ins), sum(nret[k] for k in oos)
        if n_is == 0 or n_oos == 0:
            cnt["n_dead"] += 1
            picks.append((-1, 0, 0.0, 0.0))
            equals.append(0)
            continue
        IS = [N._sharpe(sum(s1[p][k] for k in ins), sum(s2[p][k] for k in ins), n_is + 1, ann) for p in range(P)]
        OOS = [N._sharpe(sum(s1[p][k] for k in oos), sum(s2[p][k] for k in oos), n_oos + 1, ann) for p in range(P)]
        ki, ko = [key(x) for x in IS], [key(x) for x in OOS]
        best = ki.index(max(ki))            # ties to the lowest p
        below = sum(ko[q] < ko[best] for q in range(P))
        equal = sum(q != best and ko[q] == ko[best] for q in range(P))
        r2 = 2 * below + equal
        cnt["n_live"] += 1
        cnt["n_overfit"] += r2 <= P - 1
        cnt["n_loss"] += sum(s1[best][k] for k in oos) < 0
        cnt["n_tied"] += ki.count(ki[best]) > 1
        hist[r2] += 1
        picks.append((best, r2, IS[best], OOS[best]))
        equals.append(equal)
    return cnt, hist, picks, equals


def ref_cscv(folds, sym_ids, ann):
    """(groups CSCV_GROUP_DTYPE[G], hist uint32[G, 2P - 1], picks CSCV_PICK_DTYPE[G, C]) of fold
    records folds[G, P, K]; sym_ids None: group g reports sym = g."""
    G, P, K = folds.shape
    groups = np.zeros(G, D.CSCV_GROUP_DTYPE)
    hist = np.zeros((G, 2 * P - 1), np.uint32)
    picks = np.zeros((G, len(masks(K))), D.CSCV_PICK_DTYPE)
    for g in range(G):
        cnt, h, pk, _ = ref_group(folds[g], ann)
        groups[g]["sym"] = g if sym_ids is None else sym_ids[g]
        groups[g]["n_lanes"] = P
        for name, v in cnt.items():
            groups[g][name] = v
        hist[g] = h
        for c, (lane, r2, a, b) in enumerate(pk):
            picks[g, c] = (lane, r2, a, b)
    return groups, hist, picks


# ------------------------------------------------------------------------------ crafted records
def crafted(K, P, G, seed):
    """Fold records no backtest produces (FOLD_DTYPE[G, P, K]), seeded: s1 of both signs at
    magnitudes 2^63 .. 2^119 so that carries cross the words in the half sums and in total minus
    half, duplicate lanes, all-zero lanes, lanes whose s2 is so small that the variance is not
    positive, folds without return bars in some groups and, in the last group of a call with
    G >= 2, bars in the fold of bit K - 1 only."""
    import random
    rng = random.Random(seed * 1000003 + K * 1009 + P * 17 + G)
    f = np.zeros((G, P, K), D.FOLD_DTYPE)
    for g in range(G):
        first = 0
        nb = [rng.choice([1, 2, 5, 40, 300]) for _ in range(K)]
        if g % 3 == 1:                       # some folds without return bars
            for k in rng.sample(range(K), max(1, K // 2)):
                nb[k] = 0
            nb[0] = 1                        # bar 0 alone: a fold with a bar and no return bar
        if G >= 2 and g == G - 1:            # only bit K - 1's fold has bars: every combination dead
            nb = [0] * (K - 1) + [50]
        for k in range(K):
            f[g, :, k]["first_bar"] = first
            f[g, :, k]["n_bars"] = nb[k]
            first += nb[k]
        for p in range(P):
            kind = rng.randrange(6)
            for k in range(K):
                if kind == 0 or nb[k] == 0 or n_ret(int(f[g, p, k]["first_bar"]), nb[k]) == 0:
                    s1 = s2 = 0              # an all-zero lane, or a fold without return bars
                elif kind == 1:              # s2 far too small for its s1: v <= 0
                    s1 = rng.choice([-1, 1]) * rng.randrange(1 << 60, 1 << 70)
                    s2 = rng.randrange(0, 4)
                else:
                    e = rng.choice([63, 64, 65, 100, 118, 119])
                    s1 = rng.choice([-1, 1]) * rng.randrange(1 << (e - 1), 1 << e) if e < 119 else \
                        rng.choice([-1, 1]) * ((1 << 120) - 1 - rng.randrange(1 << 20))
                    s1 = rng.choice([s1, s1, (1 << 64) - 1, -(1 << 64), 1 << 64, -1])
                    s2 = rng.choice([rng.randrange(1 << 100, 1 << 120), (1 << 120) - 1, (1 << 64) - 1, 1 << 64,
                                     rng.randrange(1, 1 << 64)])
                f[g, p, k]["s1_lo"], f[g, p, k]["s1_hi"] = s1 & ((1 << 64) - 1), s1 >> 64
                f[g, p, k]["s2_lo"], f[g, p, k]["s2_hi"] = s2 & ((1 << 64) - 1), s2 >> 64
        for p in range(1, P):                # duplicate lanes: in-sample ties, equal > 0
            if rng.randrange(3) == 0:
                src = rng.randrange(p)
                for name in ("s1_lo", "s1_hi", "s2_lo", "s2_hi"):
                    f[g, p][name] = f[g, src][name]
    return f
