"""Covariance of chosen lanes, the parts that need no GPU (docs/covariance_spec.md):
bt_covariance_host against the reference of gram_ref.py byte for byte, its refusals and those of the
entry points that take an engine, the planner (plan_gram through tests/plan/gram_plan_driver.cpp)
and the host code as a stand-alone program under AddressSanitizer and UBSan
(tests/asan/gram_driver.cpp)."""
import os
import re
import subprocess

import numpy as np
import pytest

import dbx_amd as D
from dbx_amd import engine as E
import gram_ref as G
from helpers import CSRC, ROOT, SANITIZE, SANITIZE_ENV, assert_staging_layout, build_plan_driver, run_driver

STRATEGIES = ("sma", "ema_ols", "boll")


# ---------------------------------------------------------- (a) the host restatement, byte for byte
@pytest.mark.parametrize("strategy", STRATEGIES)
def test_host_equals_the_reference_on_the_edge_set(strategy):
    _, lanes, curves = G.edge_lanes(strategy)
    assert len(lanes) == 21 and len(set(lanes)) == 20 and sorted(len(c) for c in curves)[0] == 1
    eq, nb = G.curve_arrays(curves, 1000)
    for window in G.WINDOWS:
        want = G.edge_reference(strategy, window)
        G.assert_equal(D.covariance_host(eq, nb, window), want, f"{strategy} window {window}")
    gram, sums, T = G.edge_reference(strategy, (0, G.WHOLE))
    assert T == 1000 and G.edge_reference(strategy, (63, 65))[2] == 2 and G.edge_reference(strategy, (5, 5))[2] == 0
    assert any(int(gram[i, i]) > 0 for i in range(21)) and sums.any(), "the lanes trade"
    # the lane given twice: equal rows and columns
    i, j = [k for k, L in enumerate(lanes) if L == (650, 4)]
    assert all(gram[i, k] == gram[j, k] for k in range(21)) and gram[i, j] == gram[i, i]
    # short symbols contribute zeros after their end: the one-bar lane has no bar in [500, 1000)
    tail = G.edge_reference(strategy, (500, 1000))[0]
    short = [k for k, c in enumerate(curves) if len(c) <= 500]
    assert len(short) >= 16 and all(tail[k, m] == 0 for k in short for m in range(21))


def test_windows_add_and_the_default_window_is_every_bar():
    _, _, curves = G.edge_lanes("sma")
    eq, nb = G.curve_arrays(curves, 1000)
    whole = D.covariance_host(eq, nb)
    assert whole.n_bars == 1000
    G.assert_equal(whole, G.edge_reference("sma", (0, G.WHOLE)), "no window")
    for a in (1, 64, 333):
        lo, hi = D.covariance_host(eq, nb, (0, a)), D.covariance_host(eq, nb, (a, 1000))
        assert lo.n_bars + hi.n_bars == 1000
        assert np.array_equal(lo.gram + hi.gram, whole.gram) and np.array_equal(lo.sums + hi.sums, whole.sums)
    # the book's second moment: w^T gram w, all ones by default
    g = whole.gram
    assert whole.book_s2() == sum(int(x) for x in g.reshape(-1))
    w = list(range(-10, 11))
    assert whole.book_s2(w) == sum(w[i] * w[j] * int(g[i, j]) for i in range(21) for j in range(21))
    with pytest.raises(ValueError, match="integer weight"):
        whole.book_s2([0.5] * 21)
    # the float views: one rounding per entry, then the operations in the order written
    f = whole.gram_f64
    assert all(f[i, j] == float(int(g[i, j])) for i in range(21) for j in range(21))
    m = whole.sums.astype(np.float64) / 1000.0
    assert np.array_equal(whole.cov(), f / 1000.0 - np.outer(m, m))
    v = np.diagonal(whole.cov())
    assert np.array_equal(whole.vol(), np.sqrt(np.where(v > 0, v, 0.0)))
    c = whole.corr()
    flat = [k for k in range(21) if not v[k] > 0]
    assert flat and not c[flat].any() and np.allclose(np.diagonal(c)[v > 0], 1.0) and np.abs(c).max() <= 1 + 1e-12
    none = D.covariance_host(np.zeros((0, 4), np.int64), [])
    assert none.n_bars == 0 and none.gram.shape == (0, 0) and none.cov().shape == (0, 0) and none.book_s2() == 0


# -------------------------------------------------------------------------------- (b) refusals
def test_refusals_name_the_value_and_leave_the_library_usable():
    _, _, curves = G.edge_lanes("sma")
    want = G.edge_reference("sma", (64, 128))
    eq, nb = G.curve_arrays(curves, 1000)
    n = len(curves)
    host = E.sym("bt_covariance_host")
    wide, sums, T = np.zeros(n * n, D.WIDE_DTYPE), np.zeros(n, np.int64), np.zeros(1, np.int32)
    out = (wide.ctypes.data, sums.ctypes.data, T.ctypes.data)

    def last():
        return D.lib().bt_last_error().decode()

    def still_good():
        assert host(n, eq.ctypes.data, nb.ctypes.data, 1000, 64, 128, *out) == 0
        G.assert_equal(D.Covariance(wide.reshape(n, n), sums, int(T[0])), want, "after a refusal")

    long_ = nb.copy()
    long_[3] = 1001
    e, b = eq.ctypes.data, nb.ctypes.data
    for args, named in (
        ((-1, e, b, 1000, 0, 10, *out), r"bt_covariance_host: n = -1 outside \[0, 2048\]"),
        ((2049, e, b, 1000, 0, 10, *out), r"n = 2049 outside \[0, 2048\]"),
        ((n, e, b, 1000, -4, 10, *out), r"from_bar = -4 is negative"),
        ((n, e, b, 1000, 9, 8, *out), r"to_bar = 8 is below from_bar = 9"),
        ((n, e, b, 1000, 0, 10, None, None, None), r"gram, sums and T are all NULL"),
        ((n, None, b, 1000, 0, 10, *out), r"equity and n_bars are required"),
        ((n, e, None, 1000, 0, 10, *out), r"equity and n_bars are required"),
        ((n, e, b, -1, 0, 10, *out), r"stride = -1 is negative"),
        ((n, e, long_.ctypes.data, 1000, 0, 10, *out), r"n_bars = 1001 outside \[0, stride = 1000\] \(lane 3\)"),
    ):
        assert host(*args) == -1
        assert re.search(named, last()), last()
        still_good()
    # T > 2^22: one lane of 2^22 + 1 bars, window one bar shorter is legal
    big = np.zeros((1, (1 << 22) + 1), np.int64)
    bars = np.array([(1 << 22) + 1], np.int32)
    one = np.zeros(1, D.WIDE_DTYPE)
    assert host(1, big.ctypes.data, bars.ctypes.data, big.shape[1], 0, 2**31 - 1, one.ctypes.data, None, None) == -1
    assert re.search(r"T = 4194305 bars of the window \[0, 4194305\) above 2\^22", last()), last()
    assert host(1, big.ctypes.data, bars.ctypes.data, big.shape[1], 1, 2**31 - 1, one.ctypes.data, None, T.ctypes.data) == 0
    assert int(T[0]) == 1 << 22
    # the entry points that take an engine refuse a null one
    assert E.sym("bt_covariance")(None, 0, None, 0, 10, *out) == -1
    assert re.search(r"bt_covariance: null engine", last()), last()
    assert E.sym("bt_gram_of")(None, 0, 0, None, out[0], out[1]) == -1
    assert re.search(r"bt_gram_of: null engine", last()), last()
    assert E.sym("bt_set_gram_split")(None, 0) == -1
    assert re.search(r"bt_set_gram_split: null engine", last()), last()
    still_good()
    with pytest.raises(ValueError, match="window"):
        D.covariance_host(eq, nb, (0, 1, 2))
    with pytest.raises(ValueError, match="n x stride"):
        D.covariance_host(eq, nb[:5])


# --------------------------------------------------------------------------------- (c) planner
@pytest.fixture(scope="module")
def plan():
    exe = build_plan_driver("gram_plan_driver")

    def run(n, T, cus=256, split=0):
        return run_driver(exe, n, T, cus, split)
    return run


def _regions(pl, n):
    return [(pl["o_lanes"], n * pl["lane_bytes"]), (pl["o_d"], n * pl["pitch"] * 4),
            (pl["o_partial"], pl["chunks"] * pl["tiles"] * 256 * pl["wide_bytes"]),
            (pl["o_gram"], n * n * pl["wide_bytes"]), (pl["o_sums"], n * 8)]


PLAN_SHAPES = {"one": (1, 1), "odd": (17, 65), "config2": (2048, 2520), "config5": (64, 491400), "longest": (2, 1 << 22)}


@pytest.mark.parametrize("split", (0, 1, 2, 7, 100000))
@pytest.mark.parametrize("name", list(PLAN_SHAPES))
def test_plan_gram_layout(plan, name, split):
    n, T = PLAN_SHAPES[name]
    pl = plan(n, T, split=split)
    assert pl == plan(n, T, split=split), "the plan is a function of its arguments"
    assert pl["lane_bytes"] == 16 and pl["wide_bytes"] == 16 and pl["staging_max"] == 256 << 20
    assert pl["pitch"] % 64 == 0 and T <= pl["pitch"] < T + 64
    assert pl["nt"] == (n + 15) // 16 and pl["tiles"] == pl["nt"] * (pl["nt"] + 1) // 2
    assert_staging_layout(_regions(pl, n), pl["staging_bytes"], f"{name} split {split}")
    assert pl["staging_bytes"] <= 256 << 20, "the shapes of the issue fit the arena"
    assert pl["d_bytes"] >= n * pl["pitch"] * 4 and pl["o_d"] + pl["d_bytes"] <= pl["o_partial"]
    assert pl["out_bytes"] == pl["o_sums"] + n * 8 - pl["o_gram"], "gram and sums come back in one copy"
    # the chunks: whole 64-bar groups, none empty, together the pitch; the partials within their budget
    chunks, per = pl["chunks"], pl["chunk_bars"]
    assert per % 64 == 0 and chunks >= 1 and (chunks - 1) * per < pl["pitch"] <= chunks * per
    assert chunks == 1 or chunks * pl["tiles"] * 4096 <= pl["partial_budget"]
    if split:   # a forced count: honoured up to one chunk per group and the budget, empty chunks dropped
        groups = pl["pitch"] // 64
        most = min(split, groups, max(1, pl["partial_budget"] // (pl["tiles"] * 4096)))
        assert chunks == -(-groups // -(-groups // most))
    assert pl["fold_block"] % 64 == 0


def test_plan_gram_splits_a_small_n_with_a_long_T_and_not_a_large_n(plan):
    assert plan(2048, 2520)["chunks"] == 1 and plan(256, 2520)["chunks"] <= 5
    wide_ = plan(64, 491400)
    assert wide_["tiles"] == 10 and wide_["chunks"] * 10 >= 256 * 8 * 0.95 and wide_["chunk_bars"] >= 512
    assert wide_["fill"] == pytest.approx(wide_["chunks"] * 10 / 2048)
    assert plan(2, 1 << 22)["chunks"] >= 2000 and plan(2, 1 << 22)["staging_bytes"] < 48 << 20
    assert plan(17, 65)["chunks"] == 1 and plan(17, 65, split=2)["chunks"] == 2 and plan(17, 65, split=7)["chunks"] == 2
    assert plan(33, 1000, split=7)["chunks"] in (6, 7) and plan(33, 1000, split=2)["chunks"] == 2
    assert plan(64, 491400, cus=8)["chunks"] < wide_["chunks"]
    # what does not fit is the call's to refuse: the plan still reports its need
    assert plan(2048, 1 << 22)["staging_bytes"] > 256 << 20
    assert plan(0, 0)["staging_bytes"] == 256 and plan(0, 0)["chunks"] == 1


def test_plan_driver_under_asan_and_ubsan():
    exe = build_plan_driver("gram_plan_driver", sanitize=True)
    for args in ((17, 65, 256, 0), (64, 491400, 304, 7), (0, 0, 1, 0), (2048, 1 << 22, 256, 0)):
        assert run_driver(exe, *args, sanitized=True) == run_driver(build_plan_driver("gram_plan_driver"), *args)


# ---------------------------------------------------------------------- (d) under the sanitizers
def test_host_code_under_asan_and_ubsan(tmp_path):
    """csrc/covariance.cpp and plan.cpp as a program of their own."""
    exe = str(tmp_path / "gram_asan")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", *SANITIZE,
                        "-x", "hip", "--cuda-host-only", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "asan", "gram_driver.cpp"), os.path.join(CSRC, "covariance.cpp"),
                        os.path.join(CSRC, "plan.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    for strategy, window in (("sma", (0, G.WHOLE)), ("boll", (63, 65)), ("ema_ols", (500, 1000)), ("sma", (5, 5))):
        _, _, curves = G.edge_lanes(strategy)
        want = G.edge_reference(strategy, window)
        eq, nb = G.curve_arrays(curves, 1000)
        n = len(curves)
        fin, fout = str(tmp_path / "in"), str(tmp_path / "out")
        with open(fin, "wb") as f:
            f.write(np.array([n, 1000, *window], np.int32).tobytes() + nb.tobytes() + eq.tobytes())
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, env=SANITIZE_ENV, timeout=120)
        assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
        raw = open(fout, "rb").read()
        assert len(raw) == n * n * 16 + n * 8 + 4
        got = D.Covariance(np.frombuffer(raw[:n * n * 16], D.WIDE_DTYPE).reshape(n, n),
                           np.frombuffer(raw[n * n * 16:n * n * 16 + n * 8], np.int64),
                           int(np.frombuffer(raw[-4:], np.int32)[0]))
        G.assert_equal(got, want, f"{strategy} window {window} under the sanitizers")
        lines = r.stdout.splitlines()
        assert lines[-1] == f"ok {n} {want[2]}"
        refused = [ln for ln in lines if ln.startswith("refused: ")]
        assert len(refused) == 8
        for ln, named in zip(refused, ("n = -1 ", "n = 2049 ", "from_bar = -3 is negative", "to_bar = 6 is below from_bar = 7",
                                       "all NULL", "equity and n_bars are required", "n_bars = 3 outside [0, stride = 2] (lane 0)",
                                       "stride = -1 is negative")):
            assert named in ln, ln
        rules = [ln[len("rule: "):] for ln in lines if ln.startswith("rule: ")]
        assert rules == [
            "no dataset loaded", "lanes are required", "",
            "T = 4194305 bars of the window [1, 4194306) above 2^22", "", "",
            "n = -1 outside [0, 2048]", "T = 4194305 outside [0, 4194304]", "d is required", "gram and sums are both NULL", "",
            "d[1][1] = -2147483648 outside the domain |d| < 2^31", "",
            rules[13], ""]
        assert re.fullmatch(r"n = 2048 lanes over T = 4194304 bars need \d{11} bytes of device staging, above 268435456", rules[13])
        assert [ln for ln in lines if ln.startswith("window: ")] == ["window: 4194304", "window: 0"]
        assert len([ln for ln in lines if ln.startswith("plan: ")]) == 8 * 5
