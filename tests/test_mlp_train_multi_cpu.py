"""The condition that gives tolerance 0 a meaning for the multi-network training cases
(tests/mlp_train_multi_cases.py), without a GPU: for every (shape, seed) pair the GPU test compares with
np.array_equal, every partial sum of the forward and of the backward is exactly representable in f32 in
any order -- the forward's worst sums and backward_worst stay below mlp_exact_cases.LIMIT -- and every
gradient is a whole number of quarter grains that fits f32 exactly.  And the three seeds' first-layer
gradients differ from each other, so a launch that routes a job to another network's pointers shows."""
import numpy as np
import pytest

import mlp_exact_cases as mx
import mlp_grad_cases as mg
import mlp_train_multi_cases as mm

GRADS = mm.KEYS


@pytest.mark.parametrize("k", range(3))
@pytest.mark.parametrize("variant,rows", mm.SHAPES, ids=lambda v: str(v))
def test_sums_stay_exact_in_f32(variant, rows, k):
    w, x, d, fwd, ref = mm.job(variant, rows, k)
    mref = mx.reference(w, x, "f32")
    assert np.array_equal(fwd["h0"], mref["h1"]) and np.array_equal(fwd["h1"], mref["h2"])
    assert np.array_equal(fwd["logits"], mref["logits"])
    assert max(mref["worst"]) < mx.LIMIT, mref["worst"]
    assert d.shape == (rows, 9) and set(np.unique(d)) <= {-2, -1, 0, 1, 2} and d.any()
    assert np.array_equal(d, np.random.default_rng([41, mm.SEEDS[k], rows]).integers(-2, 3, (rows, 9)))
    worst = mg.backward_worst(w, x, d, fwd)
    print(variant, rows, "seed", mm.SEEDS[k], "worst backward sums in grains of 2^-2:",
          {kk: "%.3g" % v for kk, v in worst.items()})
    assert max(worst.values()) < mx.LIMIT, worst
    for g in GRADS:
        assert np.array_equal(ref[g] * 4, np.round(ref[g] * 4)), g
        assert np.array_equal(ref[g].astype(np.float32).astype(np.float64), ref[g]), g


@pytest.mark.parametrize("variant,rows", mm.SHAPES, ids=lambda v: str(v))
def test_the_fourth_job_is_the_single_network_case(variant, rows):
    assert (variant, rows) in mg.EXACT_CASES     # its condition is held by tests/test_mlp_grad_cpu.py
    assert mm.job(variant, rows, 3) is mg.exact_case(variant, rows)


@pytest.mark.parametrize("variant,rows", mm.SHAPES, ids=lambda v: str(v))
def test_the_jobs_differ_from_each_other(variant, rows):
    jobs = [mm.job(variant, rows, k) for k in range(4)]
    for a in range(4):
        for b in range(a):
            assert not np.array_equal(jobs[a][4]["w0"], jobs[b][4]["w0"]), (a, b, "gW0")
            assert not np.array_equal(jobs[a][0]["w0"], jobs[b][0]["w0"]), (a, b, "W0")
            assert not np.array_equal(jobs[a][3]["logits"], jobs[b][3]["logits"]), (a, b, "logits")


def test_real_jobs_share_one_input_between_the_first_two():
    for variant, rows in mm.REAL_SHAPES:
        x = [mm.real_job(variant, rows, k)[1] for k in range(4)]
        assert np.array_equal(x[0], x[1]) and not np.array_equal(x[1], x[2]) and not np.array_equal(x[2], x[3])
        w = [mm.real_job(variant, rows, k)[0] for k in range(4)]
        assert all(not np.array_equal(w[a]["w1"], w[b]["w1"]) for a in range(4) for b in range(a))
