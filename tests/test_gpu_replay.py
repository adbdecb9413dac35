"""The replay ring on the GPU (k_replay_put / k_replay_gather, csrc/replay.h; warehouse.ReplayBuffer),
at tolerance 0 against the oracle's rows of the captured states.  The bodies live in
tests/replay_cases.py; tests/test_replay_cpu.py runs the same bodies on the host engine."""
import pytest

import replay_cases as rc

pytestmark = pytest.mark.gpu


def _factory(**fixed):
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    import warehouse

    def factory(variant, num_envs, num_agents=None, **kw):
        return warehouse.BatchedWarehouse(variant, num_envs, num_agents, **fixed, **kw)

    return factory


@pytest.fixture(scope="module")
def make():
    return _factory(device="cuda:0")


@pytest.fixture(scope="module")
def make_host():
    return _factory(device="cpu")


@pytest.mark.parametrize("variant,na,train", rc.VARIANTS, ids=rc.IDS)
def test_round_trip_against_the_oracle(make, variant, na, train):
    rc.case_round_trip(make, variant, na, train)


@pytest.mark.parametrize("full", [True, False], ids=["full", "sparse"])
@pytest.mark.parametrize("variant,na,train", rc.VARIANTS, ids=rc.IDS)
def test_round_trip_from_fuzzed_states(make, variant, na, train, full):
    rc.case_round_trip_fuzzed(make, variant, na, train, full)


@pytest.mark.parametrize("variant,na,train", [("medium", 8, False), ("medium", None, True)], ids=["medium8", "medium_train"])
def test_step_leaves_the_trajectory_alone(make, variant, na, train):
    rc.case_step_keeps_trajectory(make, variant, na, train)


def test_step_with_the_wide_step_form():
    """lanes_per_env=16 envs record through the same buffer (the wide vector_step, unchanged)."""
    rc.case_step_keeps_trajectory(_factory(device="cuda:0", lanes_per_env=16), "medium", 8, False)
    rc.case_round_trip(_factory(device="cuda:0", lanes_per_env=16), "small", 4, False)


def test_index_draw(make):
    rc.case_index_draw(make)


@pytest.mark.parametrize("variant,na,train", [("medium", 8, False), ("medium", 3, False), ("large", 16, False)],
                         ids=["medium8", "medium3", "large16"])
def test_invalid_indices(make, variant, na, train):
    rc.case_invalid_indices(make, variant, na, train)


@pytest.mark.parametrize("variant,na", [("medium", 8), ("medium", 1), ("medium", 9), ("large", 16)],
                         ids=["medium8", "medium1", "medium9", "large16"])
def test_fragments(make, variant, na):
    rc.case_fragments(make, variant, na)


@pytest.mark.parametrize("variant,na", [("medium", 8), ("medium", 1), ("large", 16)], ids=["medium8", "medium1", "large16"])
def test_fragments_and_rows_from_fuzzed_states(make, variant, na):
    rc.case_fragments_fuzzed(make, variant, na)


@pytest.mark.parametrize("variant,na,train", [("medium", 8, False), ("medium", None, True)], ids=["medium8", "medium_train"])
def test_ring_portability(make, make_host, variant, na, train):
    rc.case_ring_portability(make, make_host, variant, na, train)


def test_refusals_on_the_device():
    """The refusal table against the device library with a device present (B = 0 and M = 0 launch
    nothing), equal to the host engine's codes."""
    from warehouse import _native as nat

    assert rc.case_refusals(nat, nat.lib(), host=False) == rc.case_refusals(nat, nat.host_lib(), host=True)
