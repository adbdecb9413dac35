"""The host engine's wh_sac_td_la and wh_adam_step_clock under AddressSanitizer + UndefinedBehaviorSanitizer:
csrc/host_engine.cpp compiled with -fsanitize=address,undefined and linked into the stand-alone
tests/asan/sync_free_asan.cpp, which calls both with buffers of exactly the stated sizes (one float of
log_alpha, one wh_adam_clock, the segments of tests/adam_cases.py) and checks the results against the
by-value entry points bit for bit.  Nothing is preloaded.  No report, "ASAN SYNC FREE OK"."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rllib-warehouse_amd", "csrc")


@pytest.mark.timeout(600)
def test_sync_free_entry_points_under_address_and_undefined_sanitizers():
    out = os.path.join(ROOT, "build", "asan", "sync_free_asan")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-DWH_HOST_ENGINE", '-DWH_SOURCE_SHA="asan"', '-DWH_VARIANT=""',
           "-I" + os.path.join(ROOT, "include"), os.path.join(CSRC, "host_engine.cpp"),
           os.path.join(CSRC, "version.cpp"), os.path.join(ROOT, "tests", "asan", "sync_free_asan.cpp"), "-o", out]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([out], capture_output=True, text=True, timeout=300, env=env)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and "ASAN SYNC FREE OK" in r.stdout, (r.stdout + r.stderr)[-3000:]
