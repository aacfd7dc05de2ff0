"""Walk-forward evaluation, the parts that need no GPU (docs/walkforward_spec.md): the reference of
walkfwd_ref.py pinned to the C oracle's whole-series figures, bt_walk_forward_host against that
reference byte for byte, its refusals, the record layouts, the chunk planner (plan_walkfwd through
tests/plan/walkfwd_plan_driver.cpp) and the host code as a stand-alone program under
AddressSanitizer and UBSan (tests/asan/walkfwd_driver.cpp)."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import dbx_amd as D
from dbx_amd import engine as E
import orc_ffi as F
import walkfwd_ref as R
from helpers import assert_staging_layout, build_plan_driver, run_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed-backtesting-exploration_amd", "csrc")


# ------------------------------------------------------------------- (a) the reference itself
def _sum128(folds, name):
    return sum(R._join(f[name + "_lo"], f[name + "_hi"]) for f in folds)


@pytest.mark.parametrize("strategy", ("sma", "ema_ols", "boll"))
def test_partitioning_folds_sum_to_the_oracle_summary(strategy):
    """Folds that partition [0, B) add up to the oracle's summary and int128 sums, on rows whose
    bars the bounds cut at tile edges, inside tiles and nowhere (one fold)."""
    grid = R.EDGE_GRIDS[strategy]()
    traded = 0
    for (sym, B), ohlc in zip(zip(R.EDGE_IDS, R.EDGE_BARS), R.edge_series()):
        for bounds in ((0, B), tuple(b for b in R.EDGE_BOUNDS if b < B) + (B,)):
            folds, lanes = R.ref_folds(strategy, grid, [ohlc], bounds)
            assert folds["first_bar"][0, 0].tolist() == list(bounds[:-1])
            assert int(folds["n_bars"][0, 0].sum()) == B
            for p in range(grid.n_params):
                s, f = lanes[0][p][0], folds[0, p]
                where = f"{strategy} sym {sym} ({B} bars) param {p} bounds {bounds}"
                for name, orc in (("pnl", "pnl"), ("n_trades", "n_trades"), ("exposure", "exposure")):
                    assert int(f[name].sum()) == int(s[orc]), f"{where}: {name}"
                assert _sum128(f, "s1") == F.i128(s["s1_lo"], s["s1_hi"]), where
                assert _sum128(f, "s2") == F.i128(s["s2_lo"], s["s2_hi"]), where
                assert int(f["mdd"].max()) <= int(s["mdd"]), where
                if len(bounds) == 2:   # one fold is the whole series: every field is the oracle's
                    assert int(f[0]["mdd"]) == int(s["mdd"]), where
                    assert np.float64(f[0]["sharpe"]).view(np.uint64) == np.float64(s["sharpe"]).view(np.uint64), where
                traded += int(s["n_trades"])
    assert traded >= 200


@pytest.mark.parametrize("strategy,want", (("sma", (43, 32, 5, 4)), ("ema_ols", (35, 19, 3, 5)),
                                           ("boll", (55, 33, 6, 10))))
def test_edge_case_meets_the_boundaries_it_is_there_for(strategy, want):
    assert R.edge_counts(strategy) == want


# ------------------------------------------------------- (b) the host restatement, byte for byte
@pytest.mark.parametrize("train", (0, 1, 2))
def test_host_equals_the_reference_on_the_selection_shape(train):
    grid, folds, _ = R.selection_case()
    assert folds.shape == (6, 400, 6)
    steps, total, tied = R.selection_steps(train)
    got = D.walk_forward_host(folds, R.SEL_IDS, train=train, annualization=grid.annualization)
    assert got.steps.dtype == D.WF_STEP_DTYPE and got.total.dtype == D.FOLD_DTYPE
    R.assert_same(got.steps, steps, f"steps, train {train}")
    R.assert_same(got.total, total, f"totals, train {train}")
    assert np.array_equal(got.oos_sharpe().view(np.uint64), total["sharpe"].view(np.uint64))
    assert got.train_sharpe().shape == (6, 6 - max(train, 1))
    # the tie rule is exercised: many distinct picks, exact non-zero ties of 2 to 400 lanes
    picks = steps["param"][steps["param"] >= 0]
    flat = [n for row in tied for n in row]
    assert len(np.unique(picks)) >= 18, len(np.unique(picks))
    assert sum(n > 1 for n in flat) >= 5 and (steps["param"] >= 0).all()
    nz = [n for n, sh in zip(flat, steps["train_sharpe"].reshape(-1)) if n > 1 and sh != 0.0]
    assert nz and min(nz) >= 2 and max(nz) <= 400
    if train == 1:
        assert 400 in flat, "one step ties every lane"
    assert grid.param(int(picks[0])).keys() == {"f", "s"}


def test_host_on_the_edge_rows_with_empty_folds_and_windows():
    """Rows of 1 to 1,000 bars under bounds past most of them: steps without a window or without
    an out-of-sample fold carry param -1 and the empty record, and the totals skip them."""
    grid, folds, _ = R.edge_case("sma")
    for train in (0, 1, 3):
        steps, total, _ = R.ref_steps(folds, R.EDGE_IDS, train, grid.annualization)
        got = D.walk_forward_host(folds, R.EDGE_IDS, train=train, annualization=grid.annualization)
        R.assert_same(got.steps, steps, f"edge steps, train {train}")
        R.assert_same(got.total, total, f"edge totals, train {train}")
        none = steps["param"] < 0
        assert none.any() and (~none).any()
        assert not steps["oos"]["n_bars"][none].any() and not steps["train_sharpe"][none].any()
    # the 1-bar row never has a return bar: no step picks, and its total is all zero
    assert (steps["param"][0] == -1).all() and not total[0:1].view(np.uint8).any()
    # train = 1 on fold 0 = [0, 1): a window of one bar has no return bar
    steps1, _, _ = R.ref_steps(folds, R.EDGE_IDS, 1, grid.annualization)
    assert (steps1["param"][:, 0] == -1).all() and (steps1["fold"][:, 0] == 1).all()


# ----------------------------------------------------------------------------- (c) refusals
def test_host_refusals_name_the_value_and_leave_the_library_usable():
    grid, folds, _ = R.edge_case("sma")
    S, P, K = folds.shape
    ids = np.asarray(R.EDGE_IDS, np.int32)
    steps = np.zeros((S, K), D.WF_STEP_DTYPE)
    total = np.zeros(S, D.FOLD_DTYPE)
    host = E.sym("bt_walk_forward_host")
    want_steps, want_total, _ = R.ref_steps(folds, R.EDGE_IDS, 1, grid.annualization)

    def last():
        return D.lib().bt_last_error().decode()

    def still_good():
        assert host(S, P, K, 1, folds.ctypes.data, ids.ctypes.data, 98280, steps.ctypes.data, total.ctypes.data) == 0
        R.assert_same(steps.reshape(-1)[:S * (K - 1)].reshape(S, K - 1), want_steps, "after a refusal")
        R.assert_same(total, want_total, "after a refusal")

    f, i, s, t = folds.ctypes.data, ids.ctypes.data, steps.ctypes.data, total.ctypes.data
    for args, named in (
        ((-1, P, K, 1, f, i, 98280, s, t), r"bt_walk_forward_host: S = -1 "),
        ((S, 0, K, 1, f, i, 98280, s, t), r"P = 0 "),
        ((S, P, 0, 0, f, i, 98280, s, t), r"K = 0 "),
        ((S, P, 1, 0, f, i, 98280, s, t), r"K = 1: steps and total need at least 2 folds"),
        ((S, P, K, K, f, i, 98280, s, t), rf"train = {K} outside \[0, {K - 1}\]"),
        ((S, P, K, -2, f, i, 98280, s, t), r"train = -2 "),
        ((S, P, K, 1, f, i, 98280, None, None), r"steps and total are both NULL"),
        ((S, P, K, 1, None, i, 98280, s, t), r"folds and sym_ids are required"),
        ((S, P, K, 1, f, i, 0, s, t), r"annualization = 0 "),
    ):
        assert host(*args) == -1
        assert re.search(named, last()), last()
        still_good()
    assert E.sym("bt_walk_forward")(None, 2, None, 1, None, s, t) == -1
    assert re.search(r"bt_walk_forward: null engine", last()), last()
    assert E.sym("bt_set_walkfwd_budget")(None, 0) == -1
    assert re.search(r"bt_set_walkfwd_budget: null engine", last()), last()
    still_good()
    with pytest.raises(D.BtError, match="train = 10 "):
        D.walk_forward_host(folds, R.EDGE_IDS, train=10)
    with pytest.raises(ValueError, match="sym_ids"):
        D.walk_forward_host(folds, [1, 2])
    with pytest.raises(ValueError, match="S x P x K"):
        D.walk_forward_host(folds[0], [1])


# ------------------------------------------------------------------------------------ layout
def test_record_layouts(tmp_path):
    assert D.FOLD_DTYPE.itemsize == 80 and D.WF_STEP_DTYPE.itemsize == 104
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "layout.c"
    lines = ['    printf("{\\"bt_fold\\": %d, \\"bt_wf_step\\": %d", (int)sizeof(bt_fold), (int)sizeof(bt_wf_step));\n']
    for st, dt in (("bt_fold", D.FOLD_DTYPE), ("bt_wf_step", D.WF_STEP_DTYPE)):
        lines += [f'    printf(", \\"{st}.{f}\\": %d", (int)offsetof({st}, {f}));\n' for f in dt.names]
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bt.h"\nint main(void) {\n' + "".join(lines) +
                   '    printf("}\\n");\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    r = subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(subprocess.run([exe], capture_output=True, text=True, check=True).stdout)
    assert got.pop("bt_fold") == 80 and got.pop("bt_wf_step") == 104
    want = {f"bt_fold.{f}": D.FOLD_DTYPE.fields[f][1] for f in D.FOLD_DTYPE.names}
    want.update({f"bt_wf_step.{f}": D.WF_STEP_DTYPE.fields[f][1] for f in D.WF_STEP_DTYPE.names})
    assert got == want


# ------------------------------------------------------------------------------ (d) planner
@pytest.fixture(scope="module")
def plan():
    exe = build_plan_driver("walkfwd_plan_driver")

    def run(S, P, K, bars=2520, cus=256, budget=0):
        return run_driver(exe, S, P, K, bars, cus, budget)
    return run


BUDGET = 256 << 20
PLAN_SHAPES = {
    "config2": (5000, 400, 10, 2520, 0), "one_long_row": (1, 400, 10, 1 << 22, 0), "config3": (64, 64, 12, 49140, 0),
    "config5_many_folds": (10000, 1024, 100, 49140, 0), "one": (1, 1, 1, 64, 0), "small_budget": (9, 12, 10, 1000, 40000),
    "one_row_chunks": (6, 400, 6, 600, 6 * 400 * 80 + 4096), "fits_whole": (6, 400, 6, 600, 0),
}


@pytest.mark.parametrize("name", list(PLAN_SHAPES))
def test_plan_walkfwd_covers_every_row_once_within_the_budget(plan, name):
    S, P, K, bars, req = PLAN_SHAPES[name]
    pl = plan(S, P, K, bars, 256, req)
    assert pl == plan(S, P, K, bars, 256, req), "the plan is a function of its arguments"
    assert pl["budget"] == BUDGET and pl["fold_bytes"] == 80 and pl["step_bytes"] == 104
    budget = req or BUDGET
    assert pl["row_bytes"] == K * P * 80 + (K - 1) * 104
    assert pl["bounds_bytes"] >= (K + 1) * 4 and pl["bounds_bytes"] % 256 == 0
    rpc = pl["rows_per_chunk"]
    assert 1 <= rpc <= S
    # the engine allocates staging_bytes: the plan's own regions (the bounds, a full chunk's records
    # and steps) lie inside them, and they inside the budget
    assert pl["o_rec"] == pl["bounds_bytes"]
    assert_staging_layout([(0, (K + 1) * 4), (pl["o_rec"], rpc * K * P * 80), (pl["o_steps"], rpc * (K - 1) * 104)],
                          pl["staging_bytes"], name)
    assert pl["staging_bytes"] <= budget
    # as many rows as fit: one more row would pass the budget (or there is no more row)
    assert rpc == S or pl["staging_bytes"] + pl["row_bytes"] > budget
    assert pl["chunks"] == -(-S // rpc)
    rows = pl["rows"]
    assert rows[0][0] == 0 and rows[-1][1] == S
    assert all(a[1] == b[0] for a, b in zip(rows[:-1], rows[1:]) if pl["chunks"] <= 8), "chunks are contiguous"
    assert all(0 < r1 - r0 <= rpc for r0, r1 in rows)
    assert pl["sel_block"] % 64 == 0 and 64 <= pl["sel_block"] <= 256 and pl["sel_block"] >= min(P, 256)
    assert pl["tiles"] == -(-bars // 64) and pl["waves"] == rpc * P
    assert rpc * max(P, K) <= 1 << 30


def test_plan_walkfwd_on_the_shapes_of_the_issue(plan):
    c2 = plan(5000, 400, 10)
    assert c2["chunks"] > 1 and c2["rows_per_chunk"] == (BUDGET - c2["bounds_bytes"] - 512) // c2["row_bytes"]
    assert c2["fill"] > 30                                  # a chunk fills the device many times over
    long = plan(1, 400, 10, 1 << 22)
    assert long["chunks"] == 1 and long["staging_bytes"] < (1 << 20) and long["tiles"] == 65536
    assert plan(6, 400, 6, 600, 256, 6 * 400 * 80 + 4096)["chunks"] == 6
    # one row that cannot fit: the plan says so with rows_per_chunk 0 and the call is refused
    assert plan(3, 1 << 20, 4)["rows_per_chunk"] == 0
    assert plan(3, 400, 10, 2520, 256, 1000)["rows_per_chunk"] == 0


def test_plan_driver_under_asan_and_ubsan():
    exe = build_plan_driver("walkfwd_plan_driver", sanitize=True)
    S, P, K, bars, req = PLAN_SHAPES["one_row_chunks"]
    assert run_driver(exe, S, P, K, bars, 256, req, sanitized=True) == \
        run_driver(build_plan_driver("walkfwd_plan_driver"), S, P, K, bars, 256, req)


# ---------------------------------------------------------------------- (e) under the sanitizers
def _random_folds(rng, S, P, K, empty_rows=()):
    """Self-consistent random fold records [S, P, K]: per row a bar count and common bounds give
    first_bar / n_bars; the sums are random, with exact ties and zero variances among the lanes."""
    f = np.zeros((S, P, K), D.FOLD_DTYPE)
    bounds = np.sort(rng.choice(np.arange(0, 300), K + 1, replace=False))
    bounds[0] = 0 if rng.integers(2) else bounds[0]
    for s in range(S):
        B = 0 if s in empty_rows else int(rng.integers(150, 1000))
        c = np.minimum(bounds, B)
        f["first_bar"][s] = c[:-1]
        f["n_bars"][s] = c[1:] - c[:-1]
        live = (f["n_bars"][s] > 0)[0]
        for p in range(P):
            for k in np.nonzero(live)[0]:
                r = f[s, p, k]
                if p and rng.integers(4) == 0:           # a tie with the lane before
                    f[s, p, k] = f[s, p - 1, k]
                    continue
                r["n_trades"] = rng.integers(0, 50)
                r["pnl"] = rng.integers(-2**40, 2**40)
                r["mdd"] = rng.integers(0, 2**40)
                r["exposure"] = rng.integers(0, int(r["n_bars"]) + 1)
                s2 = int(rng.integers(0, 2**62)) << int(rng.integers(0, 8))
                s1 = int(rng.integers(-2**58, 2**58)) if rng.integers(5) else 0
                (r["s1_lo"], r["s1_hi"]), (r["s2_lo"], r["s2_hi"]) = R._split(s1), R._split(s2)
                r["sharpe"] = rng.standard_normal()
    return f


ASAN_SHAPES = ((5, 7, 6, 0, ()), (4, 1, 5, 2, (1,)), (3, 130, 3, 1, (0, 2)), (0, 3, 4, 1, ()), (6, 9, 2, 0, (5,)),
               (2, 4, 9, 8, ()))


def test_host_code_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ missing")
    exe = str(tmp_path / "walkfwd_asan")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", CSRC,
                        os.path.join(ROOT, "tests", "asan", "walkfwd_driver.cpp"),
                        os.path.join(CSRC, "walkfwd.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    # verify_asan_link_order=0: the environment may preload a library ahead of the ASan runtime
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0")
    rng = np.random.default_rng(20261020)
    picked = 0
    for S, P, K, train, empty in ASAN_SHAPES:
        folds = _random_folds(rng, S, P, K, empty)
        ids = rng.integers(0, 2**31 - 1, S).astype(np.int32)
        ann = 98280
        fin, fout = str(tmp_path / f"in_{S}_{P}_{K}"), str(tmp_path / f"out_{S}_{P}_{K}")
        with open(fin, "wb") as f:
            f.write(np.array([S, P, K, train], np.int32).tobytes() + np.int64(ann).tobytes() + folds.tobytes() + ids.tobytes())
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
        n_steps = K - max(train, 1)
        raw = open(fout, "rb").read()
        ns, nt = S * n_steps * 104, S * 80
        assert len(raw) == ns + 2 * nt
        steps = np.frombuffer(raw[:ns], D.WF_STEP_DTYPE).reshape(S, n_steps)
        total = np.frombuffer(raw[ns:ns + nt], D.FOLD_DTYPE)
        alone = np.frombuffer(raw[ns + nt:], D.FOLD_DTYPE)
        want_steps, want_total, _ = R.ref_steps(folds, ids, train, ann)
        R.assert_same(steps, want_steps, f"steps {S}x{P}x{K} train {train}")
        R.assert_same(total, want_total, f"totals {S}x{P}x{K} train {train}")
        R.assert_same(alone, want_total, f"totals alone {S}x{P}x{K} train {train}")
        for s in empty:
            assert (steps["param"][s] == -1).all() and not total[s:s + 1].view(np.uint8).any()
        picked += int((steps["param"] >= 0).sum())
        lines = r.stdout.splitlines()
        assert lines[-1] == f"ok {S} {P} {K} {train}"
        refused = [ln for ln in lines if ln.startswith("refused: ")]
        assert len(refused) == 7
        for ln, named in zip(refused, ("S = -1 ", "P = 0 ", "K = 1: steps", f"train = {K} ", "train = -1 ", "both NULL",
                                       "annualization = 0 ")):
            assert named in ln, ln
        rules = [ln[len("rule: "):] for ln in lines if ln.startswith("rule: ")]
        assert rules[0] == "bounds[2] = 5 does not exceed bounds[1] = 5"
        assert rules[1] == "bounds[0] = -1 is negative"
        assert re.search(r"S\*P\*K = 4096\*513\*2 exceeds 2\^22", rules[2])
        assert rules[3] == "" and rules[4] == ""
    assert picked >= 40
