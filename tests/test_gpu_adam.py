"""wh_adam_step on the GPU (k_adam, csrc/adam.h): p, m and v equal the host engine's bit for bit after one
call at step counts 1, 2 and 1000 and after 20 chained calls with fresh gradients each, over the 24
segments of tests/adam_cases.py (counts 0 .. 300,000, aligned and misaligned), guards before and behind
every tensor.  The host engine itself is held to the float64 model and to torch by tests/test_adam_cpu.py."""
import pytest

import adam_cases as ac

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from warehouse import _native

    return _native


@pytest.mark.parametrize("t", [1, 2, 1000])
def test_one_call_equals_the_host_engine_bit_for_bit(nat, t):
    ac.case_device_equals_host(nat, t, 1)


def test_twenty_chained_calls_equal_the_host_engine_bit_for_bit(nat):
    ac.case_device_equals_host(nat, 1, 20)


def test_fewer_segments_than_the_table_holds(nat):
    ac.case_fewer_segments(nat, nat.lib(), "cuda:0")


def test_refusals_on_the_device(nat):
    assert ac.case_refusals(nat, nat.lib(), host=False) == ac.case_refusals(nat, nat.host_lib(), host=True)
