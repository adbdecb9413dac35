"""wh_sac_loss without a GPU: the bodies of tests/loss_cases.py on the host engine (the same formula header
as the device kernel, a plain loop with the sums in ascending row order), the float32 transcription of the
model, and the exact-sum case.  (The refusal table is tests/test_loss_refusals.py.)

The host engine and the float32 numpy model must stay under a QUARTER of the stated bounds on the test's
own inputs.  Largest errors seen, as fractions of the full bounds (dpi, dq, critic sums, actor sum, T):
0.031, 0.184, 0.019, 0.017, 0.0014; on the peaked-policy case 0.007, 0.177, 0.002, 0.002, 0.007
(DESIGN.md §7)."""
import pytest

import loss_cases as lc
import sac_cases as sc


@pytest.fixture(scope="module")
def nat():
    from warehouse import _native

    return _native


@pytest.mark.parametrize("M", sc.MS)
@pytest.mark.parametrize("NA", sc.NAS)
def test_losses_on_the_host_engine_against_the_float64_model(nat, NA, M):
    worst = lc.case_loss(nat, nat.host_lib(), "cpu", NA, M, quarter=True)
    print("host engine NA", NA, "M", M, "errors / bounds", worst)


@pytest.mark.parametrize("M", sc.MS)
@pytest.mark.parametrize("NA", sc.NAS)
def test_float32_model_stays_under_a_quarter_of_the_bounds(NA, M):
    worst = lc.case_float32_model(NA, M)
    print("float32 model NA", NA, "M", M, "errors / bounds", worst)


@pytest.mark.parametrize("M", sc.MS)
@pytest.mark.parametrize("NA", sc.NAS)
def test_exact_sums_on_the_host_engine(nat, NA, M):
    lc.case_exact(nat, nat.host_lib(), "cpu", NA, M)


@pytest.mark.parametrize("NA,M", [(9, 300), (8, 65)])
def test_two_calls_give_equal_bytes_on_the_host_engine(nat, NA, M):
    lc.case_deterministic(nat, nat.host_lib(), "cpu", NA, M)


def test_model_on_a_hand_worked_row():
    """One row worked by hand: a uniform policy (p = 1/9, logp = -ln 9), so f = -alpha ln 9 - mean(qm),
    dpi[j] = scale / 9 (mean(qm) - qm[j]) and t = target_entropy - ln 9."""
    import numpy as np

    q1 = np.arange(9, dtype=np.float32)[None, :]
    q2 = q1[:, ::-1].copy()
    inp = dict(pi=np.full((1, 9), 1.5, np.float32), q1=q1, q2=q2, y=np.array([[1.0]], np.float32),
               actions=np.array([[7]], np.int32), n=None, weights=np.array([0.5], np.float32))
    dpi, dq1, dq2, stats = lc.model(inp, 1, log_alpha=0.0, target_entropy=0.935, scale=0.25)
    qm = np.minimum(q1, q2)[0]
    np.testing.assert_allclose(dpi[0], 0.25 / 9 * (qm.mean() - qm), atol=1e-12)
    assert dq1[0, 7] == 0.25 * 0.5 * 6 and dq2[0, 7] == 0.25 * 0.5 * 0 and np.count_nonzero(dq1) == 1
    want = [0.25 * 0.25 * 36, 0.0, 0.25 * (-np.log(9) - qm.mean()), 0.0, -0.25 * (0.935 - np.log(9)), 1.0]
    np.testing.assert_allclose(stats, want, atol=1e-12)
