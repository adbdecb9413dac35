"""csrc/mlp_grid.h -- how wh_mlp_forward_multi shares one launch's workgroups out among its jobs --
under AddressSanitizer + UndefinedBehaviorSanitizer: the header is plain C++17, so the stand-alone
tests/asan/mlp_grid_asan.cpp includes it and g++ builds it with -fsanitize=address,undefined.  Nothing
is preloaded.  The program checks the partition's invariants for 1 to 8 jobs, caps 8, 9, 64 and 256,
task counts from {0, 1, 2, 3, C-1, C, C+1, 1000} and row counts up to 2^40, walks every job's tasks with
the kernels' job-local stride (each exactly once), and checks the f32 rule.  No report,
"ASAN MLP GRID OK"."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rllib-warehouse_amd", "csrc")


@pytest.mark.timeout(600)
def test_grid_partition_under_address_and_undefined_sanitizers():
    out = os.path.join(ROOT, "build", "asan", "mlp_grid_asan")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-I" + CSRC, os.path.join(ROOT, "tests", "asan", "mlp_grid_asan.cpp"), "-o", out]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([out], capture_output=True, text=True, timeout=300, env=env)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and "ASAN MLP GRID OK" in r.stdout, (r.stdout + r.stderr)[-3000:]
