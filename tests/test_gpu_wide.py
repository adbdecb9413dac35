"""The 16-lanes-per-env step form (lanes_per_env=16: wh_step_wide / wh_rollout_wide /
wh_vector_step_wide, csrc/step_wide.h) on the GPU, bit-exact against the reference-generated
fixtures and the fixture-pinned oracle.  The bodies live in tests/wide_cases.py; tests/test_wide_cpu.py
runs the same bodies on the host engine."""
import numpy as np
import pytest

import wide_cases as wc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def make():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    import warehouse

    def factory(variant, num_envs, num_agents=None, **kw):
        return warehouse.BatchedWarehouse(variant, num_envs, num_agents, lanes_per_env=16, **kw)

    return factory


@pytest.mark.parametrize("variant", ["small", "medium", "large"])
def test_wide_g1_reference_episodes(make, variant):
    wc.case_g1_episodes(make, variant)


@pytest.mark.parametrize("variant", ["small", "medium", "large"])
def test_wide_g2_dense_transitions(make, variant):
    wc.case_g2_dense(make, variant)


@pytest.mark.parametrize("variant", ["small", "medium", "large"])
def test_wide_fuzzed_single_transitions(make, variant):
    wc.case_fuzz(make, variant)


@pytest.mark.parametrize("variant,na,train,policy,p,staggered", wc.ROLLOUT_SHAPES)
def test_wide_fused_rollout_vs_oracle(make, variant, na, train, policy, p, staggered):
    wc.case_fused_rollout(make, variant, na, train, policy, p, staggered)


@pytest.mark.parametrize("variant,na,policy,p", wc.CO_LOCATED_SHAPES)
def test_wide_co_located_agents_vs_oracle(make, variant, na, policy, p):
    wc.case_co_located(make, variant, na, policy, p)


def test_wide_vector_step_masked_autoreset_vs_oracle(make):
    wc.case_vector_step(make)


def test_wide_shard_invariance(make):
    wc.case_shards(make)


def test_wide_edges(make):
    wc.case_edges(make)


def test_wide_refuses_order_and_split_phases(make):
    """`order=` and `phase != WH_PHASE_ALL` raise ValueError and launch nothing."""
    import torch

    env = make("medium", 6, 8, seed=1)
    env.reset()
    before = env.state.clone()
    acts = np.full((6, 8), 5, np.int32)
    order = np.tile(np.arange(8, dtype=np.int32)[::-1], (6, 1))
    with pytest.raises(ValueError, match="order"):
        env.step(acts, order=order)
    with pytest.raises(ValueError, match="phase"):
        env.step(acts, phase=1)
    with pytest.raises(ValueError, match="order"):
        env.vector_step(acts, order=order)
    torch.cuda.synchronize()
    assert torch.equal(env.state, before)
