"""The recorded step without a GPU: the bodies of tests/record_cases.py on the host engine
(wh_replay_record through drive_env), the Python surface, and the new kernels' resources."""
import os
import subprocess
import sys

import pytest
import torch

import record_cases as rec
import replay_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make(variant, num_envs, num_agents=None, **kw):
    import warehouse

    return warehouse.BatchedWarehouse(variant, num_envs, num_agents, device="cpu", **kw)


@pytest.fixture(scope="module")
def nat():
    from warehouse import _native

    return _native


@pytest.mark.parametrize("variant,na,train", rc.VARIANTS, ids=rc.IDS)
def test_ring_recorded_fused_equals_the_five_calls(variant, na, train):
    """Ring portability between the routes on the host engine: fused=True against fused=False."""
    rec.case_ring_equal(make, variant, na, train)


def test_ring_equal_with_37_envs():
    rec.case_ring_equal(make, "medium", 8, False, nb=rc.B)


@pytest.mark.parametrize("variant,na,train", rc.VARIANTS, ids=rc.IDS)
def test_ring_equal_from_fuzzed_states(variant, na, train):
    rec.case_ring_equal_fuzzed(make, variant, na, train, True)


@pytest.mark.parametrize("variant,na,train", [("medium", 8, False), ("medium", None, True), ("large", 16, False)],
                         ids=["medium8", "medium_train", "large16"])
def test_ring_equal_from_sparse_fuzzed_states(variant, na, train):
    rec.case_ring_equal_fuzzed(make, variant, na, train, False)


@pytest.mark.parametrize("policy,p", [("greedy", 0.3), ("greedy", 0.0), ("random", 0.0)],
                         ids=["greedy03", "greedy0", "random"])
@pytest.mark.parametrize("variant,na,train",
                         [("small", 4, False), ("medium", 8, False), ("medium", None, True), ("large", 16, False)],
                         ids=["small4", "medium8", "medium_train", "large16"])
def test_collect_from_fuzzed_states_against_the_oracle(variant, na, train, policy, p):
    rec.case_collect_fuzzed(make, variant, na, train, policy, p)


def test_collect_from_fuzzed_states_into_a_prioritized_buffer():
    rec.case_collect_fuzzed(make, "medium", 8, False, "greedy", 0.3, prioritized=True)


def test_collect_steps_on_after_its_own_resets():
    rec.case_collect_steps_on_after_resets(make)


@pytest.mark.parametrize("policy,p", [("greedy", 0.3), ("random", 0.0)], ids=["greedy", "random"])
@pytest.mark.parametrize("variant,na,train", [("medium", 8, False), ("medium", None, True), ("small", 4, False)],
                         ids=["medium8", "medium_train", "small4"])
def test_collect_equals_stepwise_recording(variant, na, train, policy, p):
    rec.case_collect_equal(make, variant, na, train, policy, p)


def test_collect_into_a_prioritized_buffer():
    rec.case_collect_equal(make, "medium", 8, False, "greedy", 0.3, prioritized=True)


@pytest.mark.parametrize("variant,na,train", [("medium", 8, False), ("medium", None, True), ("large", 16, False)],
                         ids=["medium8", "medium_train", "large16"])
def test_sample_after_record_against_the_oracle(variant, na, train):
    rec.case_sample_after_record(make, variant, na, train)


def test_python_surface(nat):
    import warehouse

    assert "policy_collect" in warehouse.__all__ and nat.WH_POLICY_EXTERNAL == 0
    assert "wh_replay_record" in nat.SYMBOLS
    env = make("medium", 5, 2, seed=3)
    env.reset()
    buf = warehouse.ReplayBuffer(env, 3)
    assert buf.fused is None and buf.last_fused is None
    obs, rew, done = buf.step(env.policy())
    assert buf.last_fused is True                                # None takes the record launch
    assert obs is env._obs and rew is env.rewards and done is env.dones
    with pytest.raises(ValueError, match="operand"):
        buf.step(env.policy(), operand="tiles")
    with pytest.raises(nat.WarehouseNativeError, match="fragment"):
        buf.step(env.policy(), operand="fragments")
    with pytest.raises(nat.WarehouseNativeError, match="fragment"):
        buf.collect(1, operand="fragments")
    with pytest.raises(ValueError, match="steps"):
        buf.collect(4)
    with pytest.raises(ValueError, match="steps"):
        buf.collect(-1)
    assert buf.cursor == 1 and buf.filled == 1                    # a refused call records nothing
    obs, rew, done = buf.collect(3, "random", observe=False)
    assert obs is None and rew.shape == (3, 5, 2) and done.dtype == torch.uint8
    assert buf.cursor == 1 and buf.filled == 3


def test_host_engine_refuses_the_fragment_operand(nat):
    """xfrag is WH_ENOTSUP on the host engine, after the argument checks; nothing is recorded."""
    import ctypes

    import warehouse

    env = make("small", 4, 4)
    env.reset()
    buf = warehouse.ReplayBuffer(env, 2)
    frag = torch.zeros(4096, dtype=torch.uint8)
    xf = frag.data_ptr() + (-frag.data_ptr()) % 16

    def call(slot):
        return nat.host_lib().wh_replay_record(env._cfgp, env.B, env.state.data_ptr(), ctypes.byref(buf._ring), slot, 1,
                                               1, 0.0, None, None, None, None, xf, None, 0, 0, 0, None)
    before = env.state.clone()
    assert call(0) == nat.WH_ENOTSUP
    assert call(2) == nat.WH_EINVAL
    assert torch.equal(env.state, before) and not frag.any() and not buf.states.any()


def test_record_kernels_have_no_scratch(nat):
    """tools/kernel_resources.py on the built library: 10 registry shapes x 3 policies of
    k_step_record, none with a private segment (scratch), LDS within a workgroup's 160 KB."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources as kr
    finally:
        sys.path.pop(0)
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        ks = kr.kernels(kr.code_object(nat.LIB_PATH, tmp))
    names = subprocess.run(["c++filt"], input="\n".join(k["name"] for k in ks), capture_output=True, text=True).stdout
    mine = [(k, d) for k, d in zip(ks, names.splitlines()) if "k_step_record" in d]
    assert len(mine) == 30 and len({d for _, d in mine}) == 30
    for k, _ in mine:
        assert k["scratch"] == 0 and k["lds"] <= 160 * 1024, k
