"""The host model of the policy network's action tail (oracle/policy_tail.py) on the CPU: its samples
follow softmax(z), its float32 uniform rounds as the kernel's expression does (the top 24-bit draw
gives exactly 1.0), the rows found to hit that endpoint take the action whose noise is +inf, and every
part of the counter and the key reaches the words.  All inputs are fixed: nothing is random here."""
import numpy as np
import pytest

from oracle import policy_tail as pt

SEED = 0x9E3779B97F4A7C15
ORDER = [3, 0, 7, 2, 8, 1, 5, 4, 6]      # so that no vector is monotone in the action index

VECTORS = {
    "flat": np.linspace(-0.1, 0.1, 9)[ORDER],
    "spread": np.linspace(-3.0, 3.0, 9)[ORDER],
    # action 4 near probability 1e-3: the other eight sum to about 8.3, exp(-4.8) / 8.3 = 0.99e-3
    "rare": np.array([0.3, -0.2, 0.1, 0.0, -4.8, 0.2, -0.1, 0.25, -0.3]),
}


@pytest.mark.parametrize("name", sorted(VECTORS))
def test_model_samples_follow_softmax(name):
    """2^17 rows of one logit vector: chi-square over the nine actions (bins with an expectation below
    5 merged into one) below 37.0, the p = 1e-5 quantile at 8 degrees of freedom -- fewer after a merge,
    where the same bound is only looser on the p side."""
    z = VECTORS[name].astype(np.float32)
    rows = 1 << 17
    acts, _, u = pt.gumbel_actions(np.broadcast_to(z, (rows, 9)).copy(), seed=9, step=5)
    assert u.dtype == np.float32 and (u > 0).all() and (u <= 1).all()
    p = np.exp(z.astype(np.float64) - z.max())
    p /= p.sum()
    if name == "rare":
        assert 0.8e-3 < p[4] < 1.2e-3, p[4]
    cnt = np.bincount(acts, minlength=9).astype(np.float64)
    exp = p * rows
    small = exp < 5
    if small.any():
        cnt = np.append(cnt[~small], cnt[small].sum())
        exp = np.append(exp[~small], exp[small].sum())
    chi2 = ((cnt - exp) ** 2 / exp).sum()
    print(name, "chi2", chi2, "bins", len(exp))
    assert chi2 < 37.0, chi2


def test_uniform_rounds_as_the_kernel_expression():
    w24 = np.array([0, 0x7FFFFF, 0x800000, 0x800001, 0xFFFFFE, 0xFFFFFF], np.uint64)
    want = np.array([2.0 ** -25, 0.5 - 2.0 ** -25, 0.5, 0.5 + 2.0 ** -23, 1.0 - 2.0 ** -23, 1.0])
    for low in (0, 0xFF):                                  # the low byte of the word is dropped
        u = pt.uniform_f32((w24 << np.uint64(8)) | np.uint64(low))
        assert u.dtype == np.float32
        np.testing.assert_array_equal(u.astype(np.float64), want)
    assert u[-1] == np.float32(1.0)
    np.testing.assert_allclose(want, [2.0 ** -25, 0.49999997, 0.5, 0.50000012, 0.99999988, 1.0], rtol=0, atol=6e-9)


ENDPOINTS = [(1357, 783, 3, 0xFFFFFFF1), (1388, 795, 5, 0xFFFFFF84), (2545, 1865, 3, 0xFFFFFFD8)]


@pytest.mark.parametrize("step,row,action,word", ENDPOINTS)
def test_endpoint_rows_take_the_action_whose_noise_is_infinite(step, row, action, word):
    assert int(pt.sampler_words(SEED, step, [row])[0, action]) == word
    rng = np.random.RandomState(step)
    z = (rng.standard_normal((2048, 9)) * 40).astype(np.float32)
    z[row, action] = -1e30                                 # whatever the logits are
    acts, margin, u = pt.gumbel_actions(z, SEED, step)
    assert u[row, action] == np.float32(1.0) and (u[row] == 1).sum() == 1
    assert acts[row] == action and margin[row] == np.inf
    assert pt.argmax_first(z)[row] != action
    # the same row through row0
    a1, _, u1 = pt.gumbel_actions(z[row:row + 1], SEED, step, row0=row)
    assert a1[0] == action and np.array_equal(u1[0], u[row])


def test_every_part_of_counter_and_key_reaches_the_words():
    rows = np.arange(64, dtype=np.uint64)
    base = pt.sampler_words(SEED, 7, rows)
    assert base.shape == (64, 12) and (base < (1 << 32)).all()

    def all_nine_differ(a, b):
        return bool((a[:, :9] != b[:, :9]).all())

    assert all_nine_differ(base, pt.sampler_words(SEED ^ (1 << 32), 7, rows))           # seed >> 32 only
    assert all_nine_differ(base, pt.sampler_words(SEED ^ 1, 7, rows))                   # seed & 0xffffffff only
    assert all_nine_differ(base, pt.sampler_words(SEED, 8, rows))                       # step only
    assert all_nine_differ(base, pt.sampler_words(SEED, 7, rows + np.uint64(1)))        # the row only
    assert all_nine_differ(base, pt.sampler_words(SEED, 7, rows + np.uint64(1 << 32)))  # the counter's second word
    # the 12 words of a row are three different blocks, and a seed below 2^32 has k1 = 0
    assert len({int(x) for x in base[0]}) == 12
    from oracle.philox import philox4x32_10

    blk = philox4x32_10(5, 0, 7, (5 << 24) | 2, 9, 0)
    assert [int(x) for x in pt.sampler_words(9, 7, [5])[0, 8:12]] == [int(x) for x in blk]


def test_argmax_first_and_ties_in_the_model():
    z = np.zeros((3, 9), np.float32)
    z[1, [4, 8]] = 1.0
    z[2, 8] = 1.0
    np.testing.assert_array_equal(pt.argmax_first(z), [0, 4, 8])
