"""The 16-lanes-per-env step form without a GPU: its C ABI (declared, bound, exported, argument
checks before any device call), the host engine's refusal, the Python option, the kernels' resources,
and the GPU tests' bodies (tests/wide_cases.py) run on the host engine, which checks their inputs
and the oracle against each other."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import wide_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wh_step_wide", "wh_rollout_wide", "wh_vector_step_wide")


@pytest.fixture(scope="module")
def nat():
    from warehouse import _native

    return _native


def small_cfg(nat):
    return nat.make_config(12, 4, (4, 8), 4, 200, 200)


def call_step(lib, cfg, B, lanes, state=None):
    return lib.wh_step_wide(ctypes.byref(cfg), B, state, None, None, None, None, None, 0, 0, lanes, None)


def call_rollout(lib, cfg, B, lanes, policy=1, p=0.0, steps=1, state=None):
    return lib.wh_rollout_wide(ctypes.byref(cfg), B, state, steps, policy, p, None, None, None, None, 1, 0, 0, 0,
                               lanes, None)


def call_vector(lib, cfg, B, lanes, state=None):
    return lib.wh_vector_step_wide(ctypes.byref(cfg), B, state, None, None, None, None, None, None, 1, 0, 0, 0,
                                   lanes, None)


def test_wide_entries_declared_bound_and_exported(nat):
    header = open(os.path.join(ROOT, "include", "warehouse_amd.h")).read()
    assert re.search(r"#define\s+WH_WIDE_LANES\s+16\b", header)
    assert nat.WH_WIDE_LANES == 16
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in nat.SYMBOLS
        assert hasattr(nat.lib(), name) and hasattr(nat.host_lib(), name)


def test_wide_argument_checks_need_no_device(nat):
    """Every refusal comes from host-side checks made before any device call, and an empty batch
    launches nothing, so these hold on a host without a GPU."""
    lib, cfg = nat.lib(), small_cfg(nat)
    dummy = ctypes.c_void_p(4096)   # never dereferenced: the call is refused first
    for lanes in (0, 2, 8, 32, 64):
        assert call_step(lib, cfg, 8, lanes, dummy) == nat.WH_EINVAL
        assert call_rollout(lib, cfg, 8, lanes, state=dummy) == nat.WH_EINVAL
        assert call_vector(lib, cfg, 8, lanes, dummy) == nat.WH_EINVAL
        assert call_rollout(lib, cfg, 0, lanes) == nat.WH_EINVAL
    assert call_rollout(lib, cfg, 8, 16, policy=0, state=dummy) == nat.WH_EINVAL
    assert call_rollout(lib, cfg, 8, 16, policy=3, state=dummy) == nat.WH_EINVAL
    assert call_rollout(lib, cfg, 8, 16, p=1.5, state=dummy) == nat.WH_EINVAL
    assert call_rollout(lib, cfg, 8, 16, p=float("nan"), state=dummy) == nat.WH_EINVAL
    assert call_rollout(lib, cfg, 8, 16, steps=-1, state=dummy) == nat.WH_EINVAL
    assert call_step(lib, cfg, 8, 16, dummy) == nat.WH_EINVAL        # actions missing
    assert call_vector(lib, cfg, 8, 16, dummy) == nat.WH_EINVAL      # actions missing
    assert call_step(lib, cfg, 0, 16) == nat.WH_OK
    assert call_rollout(lib, cfg, 0, 16) == nat.WH_OK
    assert call_vector(lib, cfg, 0, 16) == nat.WH_OK


def test_wide_host_engine_refuses(nat):
    lib, cfg = nat.host_lib(), small_cfg(nat)
    for lanes in (1, 16):
        assert call_step(lib, cfg, 0, lanes) == nat.WH_ENOTSUP
        assert call_rollout(lib, cfg, 0, lanes) == nat.WH_ENOTSUP
        assert call_vector(lib, cfg, 0, lanes) == nat.WH_ENOTSUP


def test_lanes_per_env_option():
    import warehouse

    with pytest.raises(ValueError, match="lanes_per_env"):
        warehouse.BatchedWarehouse("small", 4, 2, device="cpu", lanes_per_env=16)
    with pytest.raises(ValueError, match="lanes_per_env"):
        warehouse.BatchedWarehouse("small", 4, 2, device="cpu", lanes_per_env=3)
    assert warehouse.BatchedWarehouse("small", 4, 2, device="cpu").lanes_per_env == 1
    with pytest.raises(ValueError, match="lanes_per_env"):
        warehouse.vector.WarehouseVectorEnv("small", 4, 2, device="cpu", lanes_per_env=16)


def test_wide_kernels_have_no_private_segment(nat):
    """tools/kernel_resources.py on the built library: every k_step_wide instance (10 registry
    entries x 3 policies) keeps its registers, and its LDS leaves room for 2 workgroups per CU."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources as kr
    finally:
        sys.path.pop(0)
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        ks = kr.kernels(kr.code_object(nat.LIB_PATH, tmp))
    names = subprocess.run(["c++filt"], input="\n".join(k["name"] for k in ks), capture_output=True, text=True).stdout
    wide = [k for k, d in zip(ks, names.splitlines()) if "k_step_wide" in d]
    assert len(wide) == 30
    for k in wide:
        assert k["scratch"] == 0, k
        assert k["lds"] <= 80 * 1024, k


# ---- input validation of tests/test_gpu_wide.py: the same bodies on the host engine.  These pass
# without the wide form; they are here so that the inputs and the oracle are known to agree.
def host(variant, num_envs, num_agents=None, **kw):
    import warehouse

    return warehouse.BatchedWarehouse(variant, num_envs, num_agents, device="cpu", lanes_per_env=1, **kw)


@pytest.mark.parametrize("variant", ["small", "medium", "large"])
def test_inputs_g1_reference_episodes(variant):
    wc.case_g1_episodes(host, variant)


@pytest.mark.parametrize("variant", ["small", "medium", "large"])
def test_inputs_g2_dense_transitions(variant):
    wc.case_g2_dense(host, variant)


@pytest.mark.parametrize("variant", ["small", "medium", "large"])
def test_inputs_fuzzed_single_transitions(variant):
    wc.case_fuzz(host, variant)


@pytest.mark.parametrize("variant,na,train,policy,p,staggered", wc.ROLLOUT_SHAPES)
def test_inputs_fused_rollout(variant, na, train, policy, p, staggered):
    wc.case_fused_rollout(host, variant, na, train, policy, p, staggered)


@pytest.mark.parametrize("variant,na,policy,p", wc.CO_LOCATED_SHAPES)
def test_inputs_co_located_agents(variant, na, policy, p):
    wc.case_co_located(host, variant, na, policy, p)


def test_inputs_vector_step():
    wc.case_vector_step(host)


def test_inputs_shard_invariance():
    wc.case_shards(host)


def test_inputs_edges():
    wc.case_edges(host)
