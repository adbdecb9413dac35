"""wh_adam_step without a GPU: the host engine against the float64 model of the formula and against one
torch.optim.Adam step from the same state (tests/adam_cases.py, whose docstring derives the bounds), at
step counts 1, 2 and 1000, over 24 segments in one call.  Largest error / bound ratios seen: p 0.996,
m 0.64, v 0.67; torch against 4 x the bounds: p 0.49, m 0.21, v 0.13."""
import pytest

import adam_cases as ac


@pytest.fixture(scope="module")
def nat():
    from warehouse import _native

    return _native


@pytest.mark.parametrize("t", [1, 2, 1000])
def test_host_engine_against_the_float64_model_and_torch(nat, t):
    print("host engine t", t, "errors / bounds", ac.case_host_against_model(nat, t))


def test_fewer_segments_than_the_table_holds(nat):
    ac.case_fewer_segments(nat, nat.host_lib(), "cpu")


def test_adam_hyper_is_computed_in_double_and_rounded_once(nat):
    import numpy as np

    h = nat.adam_hyper(3e-4, 0.9, 0.999, 1e-8, 1000)
    assert h.beta1 == np.float32(0.9) and h.omb1 == np.float32(1.0 - 0.9) and h.omb2 == np.float32(1.0 - 0.999)
    assert h.step_size == np.float32(3e-4 / (1.0 - 0.9 ** 1000)) and h.sqrt_bc2 == np.float32(np.sqrt(1.0 - 0.999 ** 1000))
    assert h.eps == np.float32(1e-8)


def test_segments_cover_the_stated_counts_and_alignments():
    counts = [c for c, _, _ in ac.SEGMENTS]
    assert {0, 1, 3, 4, 5, 4095, 4096, 4097, 300000} <= set(counts) and len(ac.SEGMENTS) == 24
    assert any(o == 4 and g == 4 and c > 4 for c, o, g in ac.SEGMENTS)      # all four pointers at offset 4
    assert any(o == 0 and g == 4 and c > 4 for c, o, g in ac.SEGMENTS)      # g alone misaligned
