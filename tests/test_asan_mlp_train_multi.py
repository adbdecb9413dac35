"""The argument front end of the multi-network training entry points (csrc/abi_args.h:
mlp_train_multi_call) under AddressSanitizer + UndefinedBehaviorSanitizer: the stand-alone
tests/asan/mlp_train_multi_asan.cpp, compiled with -fsanitize=address,undefined, asks every rule of the
header on job arrays heap-allocated at exactly `nnets` elements, so a check that reads job `nnets` is
reported.  Nothing is preloaded and nothing runs on a GPU.  No report, "ASAN MLP TRAIN MULTI OK"."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rllib-warehouse_amd", "csrc")


def test_mlp_train_multi_front_end_under_address_and_undefined_sanitizers():
    out = os.path.join(ROOT, "build", "asan", "mlp_train_multi_asan")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           os.path.join(ROOT, "tests", "asan", "mlp_train_multi_asan.cpp"), "-o", out]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([out], capture_output=True, text=True, timeout=300, env=env)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and "ASAN MLP TRAIN MULTI OK" in r.stdout, (r.stdout + r.stderr)[-3000:]
