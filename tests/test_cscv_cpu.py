"""The probability of backtest overfitting without a GPU (docs/cscv_spec.md): bt_cscv_host against
the Python-int reference (tests/cscv_ref.py) byte for byte on the walk-forward edge set and on
crafted records, every refusal with its message, plan_cscv through its driver (staging layout,
launch cap, mask order), host code and planner under AddressSanitizer and UBSan as stand-alone
programs, the exported entry points, the identities of the outputs, and proof from the reference
alone that the cases the GPU tests run reach what the kernel can get wrong."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import cscv_ref as R
import dbx_amd as D
import walkfwd_ref as W
from dbx_amd import engine as E
from helpers import CSRC, ROOT, assert_staging_layout, build_plan_driver, run_driver

STRATEGIES = ("sma", "ema_ols", "boll")
# (K, P, G): small lane counts around every K the GPU file runs below 20
CRAFTED = ((2, 1, 3), (2, 3, 4), (4, 2, 4), (4, 5, 3), (6, 3, 3), (10, 4, 2), (16, 3, 2))
EDGE_DEAD = (252, 252, 112, 112, 42, 12, 2, 0, 0)   # per edge row, from EDGE_BOUNDS and EDGE_BARS


@functools.lru_cache(None)
def edge_ref(strategy):
    grid, folds, _ = W.edge_case(strategy)
    return R.ref_cscv(folds, W.EDGE_IDS, grid.annualization)


@functools.lru_cache(None)
def crafted_ref(K, P, G):
    return R.ref_cscv(R.crafted(K, P, G, 7), None, 252)


def same(got, want, what):
    g, h, p = want
    W.assert_same(got.groups, g, f"{what}: groups")
    assert got.hist.tobytes() == h.tobytes(), f"{what}: hist"
    W.assert_same(got.picks, p, f"{what}: picks")


# ------------------------------------------------------------------ (a) the host equals the reference
@pytest.mark.parametrize("strategy", STRATEGIES)
def test_host_equals_the_reference_on_the_edge_set(strategy):
    grid, folds, _ = W.edge_case(strategy)
    assert folds.shape == (9, 12, 10)
    got = D.cscv_host(folds, W.EDGE_IDS, grid.annualization, hist=True, picks=True)
    assert got.picks.shape == (9, 252) and got.hist.shape == (9, 23)
    same(got, edge_ref(strategy), strategy)
    assert (got.combos == np.array(R.masks(10), np.uint32)).all()


@pytest.mark.parametrize("K,P,G", CRAFTED)
def test_host_equals_the_reference_on_crafted_records(K, P, G):
    got = D.cscv_host(R.crafted(K, P, G, 7), None, 252, hist=True, picks=True)
    same(got, crafted_ref(K, P, G), f"K={K} P={P} G={G}")


def test_outputs_do_not_depend_on_which_are_asked_for():
    f = R.crafted(4, 5, 3, 7)
    full = D.cscv_host(f, [5, 3, 9], 252, hist=True, picks=True)
    assert full.groups["sym"].tolist() == [5, 3, 9]
    alone = D.cscv_host(f, [5, 3, 9], 252, hist=False, picks=False)
    assert alone.hist is None and alone.picks is None
    W.assert_same(alone.groups, full.groups, "groups alone")


# ------------------------------------------------------------------ (b) identities
@pytest.mark.parametrize("strategy", STRATEGIES)
def test_identities_of_the_outputs(strategy):
    groups, hist, picks = edge_ref(strategy)
    P, C = 12, 252
    assert (groups["n_live"] + groups["n_dead"] == C).all() and (groups["n_lanes"] == P).all()
    assert (hist.sum(axis=1) == groups["n_live"]).all()
    assert (hist[:, :P].sum(axis=1) == groups["n_overfit"]).all()   # r2 <= P - 1
    assert groups["n_dead"].tolist() == list(EDGE_DEAD)
    m = R.masks(10)
    for c in range(C):          # combination C - 1 - c is c with the halves swapped
        assert m[C - 1 - c] == ~m[c] & 1023 and (c < C // 2) == (not m[c] >> 9 & 1)
    # the pick of C - 1 - c was chosen on c's out-of-sample half: where both picks are one lane,
    # the two Sharpes are each other's
    one = (picks["lane"] == picks["lane"][:, ::-1]) & (picks["lane"] >= 0)
    assert one.any()
    assert (picks["is_sharpe"][one].view(np.uint64) == picks["oos_sharpe"][:, ::-1][one].view(np.uint64)).all()
    assert ((picks["lane"] < 0) == (picks["lane"][:, ::-1] < 0)).all()


def test_the_overfit_rule_is_the_midrank_at_most_one_half():
    from fractions import Fraction
    for P in range(1, 8):
        for r2 in range(2 * P - 1):
            w = Fraction(r2 + 2, 2 * (P + 1))
            assert 0 < w < 1 and (w <= Fraction(1, 2)) == (r2 <= P - 1)


# ------------------------------------------------------------------ (c) what the GPU cases reach
@pytest.mark.parametrize("strategy", STRATEGIES)
def test_the_edge_set_reaches_ties_level_ranks_and_both_ends(strategy):
    grid, folds, _ = W.edge_case(strategy)
    tied = level = low = high = loss = 0
    for g in range(folds.shape[0]):
        cnt, hist, picks, equals = R.ref_group(folds[g], grid.annualization)
        tied += cnt["n_tied"]
        loss += cnt["n_loss"]
        level += sum(e > 0 for e in equals)
        low += sum(lane >= 0 and r2 == 0 for lane, r2, _, _ in picks)
        high += sum(r2 == 2 * (12 - 1) for _, r2, _, _ in picks)
    print(strategy, "tied", tied, "level", level, "r2=0", low, "r2=max", high, "loss", loss)
    assert tied > 0 and level > 0 and loss > 0
    assert low > 0 and high > 0


def test_the_crafted_sets_reach_what_they_plant():
    dead_part = all_dead = tied = level = neg = big = 0
    for K, P, G in CRAFTED:
        f = R.crafted(K, P, G, 7)
        groups, hist, picks = crafted_ref(K, P, G)
        C = len(R.masks(K))
        dead_part += int(((groups["n_dead"] > 0) & (groups["n_live"] > 0)).sum())
        all_dead += int((groups["n_dead"] == C).sum())
        tied += int(groups["n_tied"].sum())
        level += int((picks["r2"] % 2 == 1).sum())     # an odd r2 has a lane level with the pick
        neg += int((f["s1_hi"] < 0).sum())
        big += int((np.abs(f["s1_hi"].astype(np.float64)) >= 2.0**54).sum())      # |s1| from 2^118
        assert (groups[-1]["n_dead"] == C) and (groups[-1]["n_live"] == 0)   # only bit K - 1's fold has bars
    assert dead_part > 0 and all_dead >= len(CRAFTED) and tied > 0 and level > 0 and neg > 0 and big > 0


# ------------------------------------------------------------------ (d) refusals
def _ok_folds(G=2, P=3, K=4):
    f = np.zeros((G, P, K), D.FOLD_DTYPE)
    f["n_bars"] = 10
    f["first_bar"] = np.arange(K) * 10
    f["s2_lo"] = 100
    return f


@pytest.mark.parametrize("edit,named", [
    (lambda f: f[:, :, :3], "K = 3 is odd"),
    (lambda f: f[:, :, :1], "K = 1 outside [2, 20]"),
    (lambda f: np.zeros((1, 1, 22), D.FOLD_DTYPE), "K = 22 outside [2, 20]"),
    (lambda f: f[:, :0], "P = 0 is below 1"),
])
def test_refusals_of_the_shape(edit, named):
    with pytest.raises(D.BtError, match="bt_cscv_host: " + named.replace("[", r"\[").replace("]", r"\]")):
        D.cscv_host(edit(_ok_folds()), None, 252)
    assert len(D.cscv_host(_ok_folds(), None, 252).groups) == 2    # the library stays usable


@pytest.mark.parametrize("field,value,named", [
    ("s2_hi", -1, r"s2 outside \[0, 2\^120\) \(group 1, lane 2, fold 3\)"),
    ("s2_hi", 1 << 56, r"s2 outside \[0, 2\^120\) \(group 1, lane 2, fold 3\)"),
    ("s1_hi", 1 << 56, r"\|s1\| is 2\^120 or more \(group 1, lane 2, fold 3\)"),
    ("s1_hi", -(1 << 56), r"\|s1\| is 2\^120 or more \(group 1, lane 2, fold 3\)"),
    ("n_bars", 11, r"first_bar, n_bars = 30, 11 differ from lane 0's 30, 10 \(group 1, lane 2, fold 3\)"),
    ("first_bar", 31, r"first_bar, n_bars = 31, 10 differ from lane 0's 30, 10 \(group 1, lane 2, fold 3\)"),
])
def test_refusals_of_a_record(field, value, named):
    f = _ok_folds()
    f[1, 2, 3][field] = value
    with pytest.raises(D.BtError, match="bt_cscv_host: " + named):
        D.cscv_host(f, None, 252)


def test_refusals_of_the_rest():
    f = _ok_folds()
    bad = f.copy()
    bad[0, :, 1]["n_bars"] = -1
    with pytest.raises(D.BtError, match=r"n_bars = -1 is negative \(group 0, lane 0, fold 1\)"):
        D.cscv_host(bad, None, 252)
    bad = f.copy()
    bad["n_bars"] = 2**30
    with pytest.raises(D.BtError, match=r"return bars in group 0 exceed 2\^31 - 2"):
        D.cscv_host(bad, None, 252)
    with pytest.raises(D.BtError, match="annualization = 0 is not positive"):
        D.cscv_host(f, None, 0)
    g = np.zeros(1, D.CSCV_GROUP_DTYPE)
    host = E.sym("bt_cscv_host")
    assert host(2, 3, 4, f.ctypes.data, None, 252, None, None, None) == -1
    assert "groups, hist and picks are all NULL" in D.lib().bt_last_error().decode()
    assert host(1, 3, 4, None, None, 252, g.ctypes.data, None, None) == -1
    assert "folds are required" in D.lib().bt_last_error().decode()
    assert host(-1, 3, 4, f.ctypes.data, None, 252, g.ctypes.data, None, None) == -1
    assert "G = -1 is negative" in D.lib().bt_last_error().decode()
    pk = np.zeros(1, D.CSCV_PICK_DTYPE)    # refused before anything is written
    assert host((1 << 22) // 6 + 1, 3, 4, f.ctypes.data, None, 252, None, None, pk.ctypes.data) == -1
    assert "G*C = 699051*6 exceeds 2^22 pick records" in D.lib().bt_last_error().decode()
    g["sym"] = 77
    assert host(0, 3, 4, None, None, 252, g.ctypes.data, None, None) == 0 and g["sym"][0] == 77   # G == 0 writes nothing
    # a null engine is refused before anything else (no GPU needed)
    assert E.sym("bt_cscv")(None, 4, None, g.ctypes.data, None, None) == -1
    assert "bt_cscv: null engine" in D.lib().bt_last_error().decode()
    assert E.sym("bt_cscv_of")(None, 1, 3, 4, f.ctypes.data, None, g.ctypes.data, None, None) == -1
    assert "bt_cscv_of: null engine" in D.lib().bt_last_error().decode()
    assert E.sym("bt_set_cscv_work")(None, 0) == -1
    assert "bt_set_cscv_work: null engine" in D.lib().bt_last_error().decode()
    with pytest.raises(ValueError, match="exactly one of bounds and folds"):
        D.Engine.cscv(None)


def test_the_entry_points_are_exported_and_late_bound():
    for name in ("bt_cscv", "bt_cscv_of", "bt_cscv_host", "bt_set_cscv_work"):
        assert name in E._LATE_SYMBOLS and E.sym(name) is not None
    hdr = open(os.path.join(ROOT, "include", "bt.h")).read()
    assert "#define BT_ABI_VERSION 3" in hdr and "int32_t bt_cscv(" in hdr
    assert D.CSCV_GROUP_DTYPE.itemsize == 32 and D.CSCV_PICK_DTYPE.itemsize == 24


def test_record_layouts_match_a_compiled_c99_host(tmp_path):
    """The two records' mirror (overfit.py CSCV_RECORDS) has the header's sizes and offsets, field by
    field, as tests/test_abi_cpu.py checks the records of records.py against tests/abi_host.c; and
    these two are the only records of the header that lie outside that table."""
    import json
    import re
    exe = str(tmp_path / "cscv_abi_host")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cscv_abi_host.c"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = json.loads(subprocess.run([exe], capture_output=True, text=True, check=True).stdout)
    assert got["abi_version"] == D.ABI_VERSION
    assert list(D.CSCV_RECORDS) == ["bt_cscv_group", "bt_cscv_pick"]
    for cname, dt in D.CSCV_RECORDS.items():
        assert got[cname] == dt.itemsize, cname
        for f in dt.names:      # every field: one the C host does not print fails here
            assert got[f"{cname}.{f}"] == dt.fields[f][1], f"{cname}.{f}"
    assert len([k for k in got if "." in k]) == sum(len(dt.names) for dt in D.CSCV_RECORDS.values())
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bt.h")).read(), flags=re.S)
    taken = set()
    for name, args in re.findall(r"\b(bt_cscv[a-z0-9_]*)\s*\(([^()]*)\)\s*;", hdr):
        taken |= set(re.findall(r"\b(bt_\w+)\s*\*", args))
    assert taken - {"bt_engine"} <= set(D.CSCV_RECORDS) | set(E.RECORDS) and set(D.CSCV_RECORDS) <= taken


# ------------------------------------------------------------------ (e) derived figures
def test_derived_figures():
    groups, hist, picks = crafted_ref(4, 5, 3)
    o = D.cscv_host(R.crafted(4, 5, 3, 7), None, 252, hist=True, picks=True)
    live = groups["n_live"].astype(float)
    want = [a / b if b else 0.0 for a, b in zip(groups["n_overfit"].tolist(), live.tolist())]
    assert o.pbo().tolist() == want and o.pbo()[-1] == 0.0        # the all-dead group: 0, not nan
    assert o.prob_loss().tolist() == [a / b if b else 0.0 for a, b in zip(groups["n_loss"].tolist(), live.tolist())]
    assert o.omega().tolist() == [(r2 + 2) / 12 for r2 in range(9)]
    assert np.allclose(o.logits(), np.log(o.omega() / (1 - o.omega()))) and (o.logits()[:5] <= 0).all()
    assert (o.logits()[5:] > 0).all()
    d = o.degradation()
    for g in range(3):
        pk = picks[g][picks[g]["lane"] >= 0]
        x, y = pk["is_sharpe"], pk["oos_sharpe"]
        if len(pk) and np.ptp(x) > 0:
            slope, icpt = np.polyfit(x, y, 1)
            assert np.allclose(d[g], [slope, icpt], rtol=1e-9, atol=1e-12 * max(1.0, np.abs(y).max()))
        else:
            assert d[g].tolist() == [0.0, 0.0]
    with pytest.raises(ValueError, match="picks were not asked for"):
        D.cscv_host(R.crafted(2, 1, 3, 7), None, 252).degradation()


# ------------------------------------------------------------------ (f) the planner
def plan(*args, sanitize=False):
    exe = build_plan_driver("cscv_plan_driver", sanitize=sanitize)
    return run_driver(exe, *args, sanitized=sanitize)


@pytest.mark.parametrize("K", [2, 4, 10, 16, 20])
def test_plan_masks_are_the_first_half_of_the_reference_order(K):
    pl = plan(1, 3, K, 0, 0, 0)
    want = R.masks(K)
    assert pl["C"] == len(want) and pl["pairs"] == len(want) // 2
    assert pl["masks"] == list(want[:len(want) // 2])
    assert all(not m >> (K - 1) & 1 for m in pl["masks"])


@pytest.mark.parametrize("G,P,K,picks,budget,work", [
    (9, 12, 10, 1, 0, 0), (9, 12, 10, 1, 0, 12 * 40), (5000, 400, 16, 0, 0, 0), (5000, 400, 10, 0, 0, 0),
    (1, 64, 16, 0, 0, 0), (1, 3, 20, 1, 0, 0), (6, 400, 6, 1, 0, 0), (7, 257, 16, 1, 0, 0), (3, 1, 2, 1, 0, 0),
    (9, 12, 10, 1, 1, 0), (100000, 2, 4, 1, 0, 0), (40, 1024, 16, 0, 1 << 26, 0),
])
def test_plan_layout_chunks_and_launch_cap(G, P, K, picks, budget, work):
    pl = plan(G, P, K, picks, budget, work)
    C = len(R.masks(K))
    where = f"G={G} P={P} K={K}"
    cap = work or pl["work"]
    if pl["rows_per_chunk"] == 0:
        assert budget and pl["row_bytes"] > budget - 2048 and pl["staging_bytes"] == 0 and pl["chunks"] == 0
        return
    assert_staging_layout([tuple(r) for r in pl["regions"]], pl["staging_bytes"], where)
    assert pl["staging_bytes"] <= (budget or pl["budget"])
    assert pl["row_bytes"] == K * P * 80 + P * (K + 1) * 32 + K * 4 + 32 + (2 * P - 1) * 4 + (C * 24 if picks else 0)
    assert pl["rows_per_chunk"] * (pl["chunks"] - 1) < G <= pl["rows_per_chunk"] * pl["chunks"]
    assert pl["block"] % 64 == 0 and 64 <= pl["block"] <= 256 and pl["rows_per_launch"] <= 65535
    # every (row, pair) of a chunk exactly once, no launch above the cap unless it is one pair
    assert pl["launches_per_row"] == -(-pl["pairs"] // pl["pairs_per_launch"])
    assert pl["launches"] == -(-pl["rows_per_chunk"] // pl["rows_per_launch"]) * pl["launches_per_row"]
    assert pl["max_cells"] <= max(cap, P) and pl["max_cells"] > 0
    if pl["launches_per_row"] > 1:
        assert pl["rows_per_launch"] == 1
    first = pl["launch_list"][0]
    assert first[0] == 0 and first[2] == 0
    last = pl["launch_list"][-1]
    assert last[0] + last[1] == pl["rows_per_chunk"] and last[3] == pl["pairs"]


def test_plan_small_work_cuts_a_row_in_three_or_more_launches():
    pl = plan(9, 12, 10, 1, 0, 12 * 40)
    assert pl["pairs"] == 126 and pl["pairs_per_launch"] == 40 and pl["launches_per_row"] == 4
    assert pl["launch_list"][:4] == [[0, 1, 0, 40], [0, 1, 40, 80], [0, 1, 80, 120], [0, 1, 120, 126]]
    one_row = plan(9, 12, 10, 1, 1, 0)       # a budget of one byte: refused, nothing planned
    assert one_row["rows_per_chunk"] == 0
    pl = plan(9, 12, 10, 1, 2048 + one_row["row_bytes"] + 1024, 0)
    assert pl["rows_per_chunk"] == 1 and pl["chunks"] == 9


def test_plan_driver_under_asan_and_ubsan():
    for args in ((9, 12, 10, 1, 0, 480), (1, 3, 20, 1, 0, 0), (5000, 400, 16, 0, 0, 0), (3, 1, 2, 1, 1, 1)):
        assert plan(*args, sanitize=True) == plan(*args)


# ------------------------------------------------------------------ (g) under the sanitizers
REFUSED = ("K = 3 is odd", "K = 0 outside", "K = 22 outside", "all NULL", "P = 0 ", "G = -1 ", "folds are required",
           "annualization = 0", "exceeds 2^22 pick records", "s2 outside", "s2 outside", "|s1| is 2^120", "|s1| is 2^120",
           "n_bars = ", "differ from lane 0's")


def test_host_code_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ missing")
    exe = str(tmp_path / "cscv_asan")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", CSRC,
                        os.path.join(ROOT, "tests", "asan", "cscv_driver.cpp"), os.path.join(CSRC, "cscv.cpp"),
                        os.path.join(CSRC, "walkfwd.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    # verify_asan_link_order=0: the environment may preload a library ahead of the ASan runtime
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0")
    grid, edge, _ = W.edge_case("sma")
    cases = [("edge", edge, W.EDGE_IDS, grid.annualization, edge_ref("sma"))]
    cases += [(f"crafted{K}_{P}", R.crafted(K, P, G, 7), None, 252, crafted_ref(K, P, G)) for K, P, G in CRAFTED[:5]]
    for name, f, ids, ann, want in cases:
        G, P, K = f.shape
        C = len(R.masks(K))
        fin, fout = str(tmp_path / f"in_{name}"), str(tmp_path / f"out_{name}")
        with open(fin, "wb") as fh:
            fh.write(np.array([G, P, K, ids is not None], np.int32).tobytes() + np.array([ann], np.int64).tobytes())
            fh.write(np.ascontiguousarray(f).tobytes())
            if ids is not None:
                fh.write(np.array(ids, np.int32).tobytes())
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
        raw = open(fout, "rb").read()
        cuts = np.cumsum([G * 32, G * (2 * P - 1) * 4, G * C * 24])
        assert len(raw) == cuts[-1]
        got = D.Overfit(K, np.frombuffer(raw[:cuts[0]], D.CSCV_GROUP_DTYPE),
                        np.frombuffer(raw[cuts[0]:cuts[1]], np.uint32).reshape(G, 2 * P - 1),
                        np.frombuffer(raw[cuts[1]:], D.CSCV_PICK_DTYPE).reshape(G, C), None)
        same(got, want, name)
        lines = r.stdout.splitlines()
        assert lines[-1] == f"ok {G} {P} {K}"
        refused = [ln for ln in lines if ln.startswith("refused: ")]
        assert len(refused) == len(REFUSED) - (P == 1)
        for ln, named in zip(refused, REFUSED):
            assert ln.startswith("refused: bt_cscv_host: ") and named in ln, ln
