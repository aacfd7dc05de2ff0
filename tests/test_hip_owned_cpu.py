"""The owning types of the host engine (csrc/hip_owned.h: DevBuf, PinnedBuf, Event, Stream) as a
stand-alone program under AddressSanitizer, UBSan and LeakSanitizer, with no HIP runtime: the
driver (tests/asan/owned_driver.cpp) defines the HIP entry points the header calls as counting
fakes, builds a holder shaped like bt_engine and fails every creating call of a scripted sequence
in turn. After the holder's scope nothing may be live and the borrowed stream is untouched."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed-backtesting-exploration_amd", "csrc")


def test_owned_resources_free_themselves_on_every_failure_path(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ missing")
    exe = str(tmp_path / "owned_asan")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall", "-Werror",
                        "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", CSRC,
                        os.path.join(ROOT, "tests", "asan", "owned_driver.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    # verify_asan_link_order=0: the environment may preload a library ahead of the ASan runtime
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    m = re.fullmatch(r"ok (\d+) creating calls\n", r.stdout)
    assert m and int(m.group(1)) == 24, r.stdout


def test_frees_are_written_in_one_place():
    """Only hip_owned.h destroys a HIP object; HIPCHK and the failure type are defined once."""
    frees = re.compile(r"hipFree|hipHostFree|hipEventDestroy|hipStreamDestroy")
    found, defs = [], []
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".cpp", ".h")):
            continue
        text = open(os.path.join(CSRC, name)).read()
        if frees.search(text):
            found.append(name)
        defs += [name] * len(re.findall(r"#define HIPCHK|struct \w+Fail\b", text))
    assert found == ["hip_owned.h"], found
    assert defs == ["hip_owned.h", "hip_owned.h"], defs
