"""The replay priority tree on the GPU (k_prio_fill / k_prio_update / k_prio_sample, csrc/prio.h;
warehouse.ReplayBuffer(prioritized=True)) at tolerance 0 against the numpy model and against the host
engine.  The bodies live in tests/prio_cases.py; tests/test_prio_cpu.py runs them on the host engine."""
import numpy as np
import pytest

import prio_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from warehouse import _native

    return _native


@pytest.fixture(scope="module")
def make():
    import warehouse

    def factory(variant, num_envs, num_agents=None, **kw):
        return warehouse.BatchedWarehouse(variant, num_envs, num_agents, device="cuda:0", **kw)

    return factory


@pytest.mark.parametrize("count", pc.COUNTS + pc.DEEP_COUNTS)
def test_fills_and_updates_against_the_model(nat, count):
    pc.case_tree_ops(nat, nat.lib(), "cuda:0", count)


@pytest.mark.parametrize("count", pc.COUNTS + pc.DEEP_COUNTS)
def test_sampling_against_the_model(nat, count):
    pc.case_sampling(nat, nat.lib(), "cuda:0", count)


@pytest.mark.parametrize("count", pc.COUNTS + pc.DEEP_COUNTS)
def test_device_and_host_engine_trees_are_byte_identical(nat, count):
    pc.case_portability(nat, count)


@pytest.mark.parametrize("variant,na", [("medium", 8), ("small", 4)], ids=["medium8", "small4"])
def test_prioritized_buffer(nat, make, variant, na):
    pc.case_buffer(make, variant, na)


def test_prioritized_buffer_of_five_levels(nat, make):
    pc.case_buffer(make, "small", 4, **pc.BIG)


def _same_on_both_engines(nat, case, *args):
    dev = case(nat, nat.lib(), "cuda:0", *args)
    host = case(nat, nat.host_lib(), "cpu", *args)
    for a, b, what in zip(dev, host, ("leaf", "node", "max_q")):
        np.testing.assert_array_equal(a, b, err_msg=what)


def test_seven_levels(nat):
    pc.case_seven_levels(nat, nat.lib(), "cuda:0")


def test_eight_levels_sparse(nat):
    pc.case_eight_levels_sparse(nat, nat.lib(), "cuda:0")


@pytest.mark.parametrize("count", (4099, 65537))
def test_wide_updates_and_samples(nat, count):
    """2^20-sample updates and 65,541-row samples against the model, and the tree they leave
    byte-identical to the host engine's."""
    _same_on_both_engines(nat, pc.case_launch_widths, count)


@pytest.mark.parametrize("count", (65537, (1 << 20) + 1))
def test_unaligned_fills_over_many_workgroups(nat, count):
    _same_on_both_engines(nat, pc.case_unaligned_fills, count)


def test_plain_buffer_has_no_tree(nat, make):
    pc.case_plain_buffer(make)


def test_refusals_on_the_device(nat):
    """The refusal table against the device library with a device present (M = 0 and n = 0 launch
    nothing), equal to the host engine's codes."""
    assert pc.case_refusals(nat, nat.lib(), host=False) == pc.case_refusals(nat, nat.host_lib(), host=True)
