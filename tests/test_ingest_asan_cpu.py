"""The host ingest (csv.cpp, payload.cpp: every Job.File byte the worker receives goes through
it) and the host half of bt_run_batch (batch.cpp: row layout, staging from 4 threads, the result
strings) under AddressSanitizer and UBSan, host code only: built with g++ next to a small driver
(tests/asan/ingest_driver.cpp) and run over generated CSV / DBXCOL1 files, valid and corrupted
(truncations, byte edits, huge bar counts, empty files). Any out-of-bounds access, overflow or
undefined behaviour aborts the driver, and so does a staged row or a string that differs from what
the driver expects."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_np as N
from dbx_amd import payload as PL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed-backtesting-exploration_amd", "csrc")


def _corpus(d):
    rng = np.random.default_rng(7)
    files = []

    def put(name, data):
        p = os.path.join(d, name)
        open(p, "wb").write(bytes(data))
        files.append(p)

    put("empty", b"")
    put("header_only", b"timestamp,open,high,low,close\n")
    put("magic_only", PL.MAGIC)
    put("huge_count", PL.MAGIC + (2 ** 31 - 1).to_bytes(4, "little") + (1).to_bytes(4, "little"))
    for s in range(12):
        o, h, lo, c, v = N.gen(s, [s], int(rng.integers(1, 400)), int(s % 2))
        for kind, blob in (("csv", N.csv_bytes(o[0], h[0], lo[0], c[0], v[0], int(s % 2))),
                           ("bin", PL.encode_columns(o[0], h[0], lo[0], c[0], v[0] if s % 3 else None))):
            put(f"{kind}{s}", blob)
            for m in range(6):
                b = bytearray(blob)
                for _ in range(int(rng.integers(1, 8))):
                    b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
                cut = int(rng.integers(0, min(64, len(b))))
                put(f"{kind}{s}_m{m}", b[:len(b) - cut] if m % 2 else b)
    return files


def test_ingest_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ missing")
    exe = str(tmp_path / "ingest_asan")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "asan", "ingest_driver.cpp"),
                        os.path.join(CSRC, "csv.cpp"), os.path.join(CSRC, "payload.cpp"),
                        os.path.join(CSRC, "batch.cpp"), "-pthread", "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    files = _corpus(str(tmp_path))
    # verify_asan_link_order=0: the environment may preload a library ahead of the ASan runtime
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0")
    r = subprocess.run([exe] + files, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    accepted = int(r.stdout.split()[1])
    assert 24 <= accepted < len(files)  # every valid file, and not the corrupted ones
