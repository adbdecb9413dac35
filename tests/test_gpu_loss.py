"""wh_sac_loss on the GPU (k_sac_loss, k_sac_loss_finish; csrc/sac_loss.h) against the float64 model of
tests/loss_cases.py within the bounds stated there, the exact-sum case bit for bit, and two calls byte for
byte.  tests/test_loss_cpu.py runs the same bodies on the host engine.

Largest errors seen on the device, as fractions of the bounds (dpi, dq, critic sums, actor sum, T):
0.030, 0.184, 0.0013, 0.0033, 0.0011; on the peaked-policy case 0.006, 0.177, 0.0005, 0.0018, 0.0001
(DESIGN.md §7)."""
import pytest

import loss_cases as lc
import sac_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from warehouse import _native

    return _native


@pytest.mark.parametrize("M", sc.MS)
@pytest.mark.parametrize("NA", sc.NAS)
def test_losses_against_the_float64_model(nat, NA, M):
    worst = lc.case_loss(nat, nat.lib(), "cuda:0", NA, M)
    print("device NA", NA, "M", M, "errors / bounds", worst)


@pytest.mark.parametrize("M", sc.MS)
@pytest.mark.parametrize("NA", sc.NAS)
def test_exact_sums(nat, NA, M):
    lc.case_exact(nat, nat.lib(), "cuda:0", NA, M)


@pytest.mark.parametrize("NA,M", [(9, 300), (8, 65)])
def test_two_calls_give_equal_bytes(nat, NA, M):
    lc.case_deterministic(nat, nat.lib(), "cuda:0", NA, M)


def test_refusals_on_the_device(nat):
    assert lc.case_refusals(nat, nat.lib(), host=False) == lc.case_refusals(nat, nat.host_lib(), host=True)
