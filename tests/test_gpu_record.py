"""The recorded step on the GPU (k_step_record, csrc/step_record.h; wh_replay_record;
ReplayBuffer(fused=...), ReplayBuffer.collect, warehouse.policy_collect), at tolerance 0 against the
five-launch route.  The bodies live in tests/record_cases.py; tests/test_record_cpu.py runs them on
the host engine."""
import pytest

import record_cases as rec
import replay_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def make():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    import warehouse

    def factory(variant, num_envs, num_agents=None, **kw):
        return warehouse.BatchedWarehouse(variant, num_envs, num_agents, device="cuda:0", **kw)

    return factory


@pytest.mark.parametrize("variant,na,train", rc.VARIANTS, ids=rc.IDS)
def test_ring_equals_the_five_launch_route(make, variant, na, train):
    rec.case_ring_equal(make, variant, na, train)


def test_ring_equal_in_one_partial_workgroup(make):
    rec.case_ring_equal(make, "medium", 8, False, nb=rc.B)


@pytest.mark.parametrize("variant,na,train", rc.VARIANTS, ids=rc.IDS)
def test_ring_equal_from_fuzzed_states(make, variant, na, train):
    rec.case_ring_equal_fuzzed(make, variant, na, train, True)


@pytest.mark.parametrize("variant,na,train", [("medium", 8, False), ("medium", None, True), ("large", 16, False)],
                         ids=["medium8", "medium_train", "large16"])
def test_ring_equal_from_sparse_fuzzed_states(make, variant, na, train):
    rec.case_ring_equal_fuzzed(make, variant, na, train, False)


@pytest.mark.parametrize("policy,p", [("greedy", 0.3), ("greedy", 0.0), ("random", 0.0)],
                         ids=["greedy03", "greedy0", "random"])
@pytest.mark.parametrize("variant,na,train",
                         [("small", 4, False), ("medium", 8, False), ("medium", None, True), ("large", 16, False)],
                         ids=["small4", "medium8", "medium_train", "large16"])
def test_collect_from_fuzzed_states_against_the_oracle(make, variant, na, train, policy, p):
    rec.case_collect_fuzzed(make, variant, na, train, policy, p)


def test_collect_from_fuzzed_states_into_a_prioritized_buffer(make):
    rec.case_collect_fuzzed(make, "medium", 8, False, "greedy", 0.3, prioritized=True)


def test_collect_steps_on_after_its_own_resets(make):
    rec.case_collect_steps_on_after_resets(make)


@pytest.mark.parametrize("policy,p", [("greedy", 0.3), ("random", 0.0)], ids=["greedy", "random"])
@pytest.mark.parametrize("variant,na,train", [("medium", 8, False), ("medium", None, True), ("small", 4, False)],
                         ids=["medium8", "medium_train", "small4"])
def test_collect_equals_stepwise_recording(make, variant, na, train, policy, p):
    rec.case_collect_equal(make, variant, na, train, policy, p)


def test_collect_into_a_prioritized_buffer(make):
    rec.case_collect_equal(make, "medium", 8, False, "greedy", 0.3, prioritized=True)


@pytest.mark.parametrize("variant,na,train", [("medium", 8, False), ("medium", None, True), ("large", 16, False)],
                         ids=["medium8", "medium_train", "large16"])
def test_sample_after_record_against_the_oracle(make, variant, na, train):
    rec.case_sample_after_record(make, variant, na, train)


@pytest.mark.parametrize("variant,na", [("medium", 8), ("small", 4)], ids=["medium8", "small4"])
def test_fragments_and_policy_collect(make, variant, na):
    rec.case_fragments(make, variant, na)


@pytest.mark.parametrize("variant,na", [("medium", 8), ("small", 4)], ids=["medium8", "small4"])
def test_policy_collect_from_fuzzed_states(make, variant, na):
    rec.case_policy_collect_fuzzed(make, variant, na)


def test_wide_envs_keep_the_five_launches():
    import warehouse

    env = warehouse.BatchedWarehouse("medium", 40, 8, device="cuda:0", lanes_per_env=16)
    env.reset()
    buf = warehouse.ReplayBuffer(env, 3, fused=True)
    buf.step(env.policy())
    assert buf.last_fused is False
    buf.collect(2)
    assert buf.last_fused is False and buf.filled == 3


def test_refusals_on_the_device():
    from warehouse import _native as nat

    assert rec.case_refusals(nat, nat.lib(), host=False) == rec.case_refusals(nat, nat.host_lib(), host=True)
