"""tests/fuzz_states.py without a GPU: the generator's RNG call order is pinned by digests taken
before it moved out of test_gpu_fuzz.py (so the fuzz tests that draw from it see the states they
always saw), and the additions -- a fixed agent count, canonical / bstate, place_fuzzed -- do what
the replay and record cases rely on."""
import hashlib

import numpy as np
import pytest

import fuzz_states as fs
from oracle import core as oc

# sha256 over the six arrays of one draw as int64 bytes: random_states(L, 64, nmax, RandomState(1000 +
# nmax)) and random_states(L, 64, nmax, RandomState(2000 + nmax), ts=[0, 5, T - 1], full=True)
DIGESTS = {
    "small": ("bf5f7e6a801efa6279a379d34d64bcea4d6aa6be55e8c9d5798a318a7de6d405",
              "e044d2ac9f5fcc5fca1ef8adc91213c03f79d729655e37842d38499e52caa7ae"),
    "medium": ("ccbba21ffbd7b39a279de9857b7881d6c071862ceef7cf0df84038a02611f334",
               "798a010afd2dcbca96fbca377662c821aa6fff8816f503e2fd9166f5930a524a"),
    "large": ("987ba8e56f39305f222a510f5ec5cdf108ff5c899c98a71e035f494061d53d03",
              "a874cfdfd84247952c3b7c73224fdc78a0b50f8a9294d0245dfc55b8920262ff"),
}


def digest(st):
    h = hashlib.sha256()
    for a in st:
        h.update(np.ascontiguousarray(a, dtype=np.int64).tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("variant", sorted(DIGESTS))
def test_generator_draws_the_states_it_always_drew(variant):
    L = oc.layout_for(variant)
    nmax = oc.VARIANTS[variant]["nmax"]
    plain = fs.random_states(L, 64, nmax, np.random.RandomState(1000 + nmax))
    full = fs.random_states(L, 64, nmax, np.random.RandomState(2000 + nmax), ts=[0, 5, L.T - 1], full=True)
    assert (digest(plain), digest(full)) == DIGESTS[variant]


def test_the_gpu_fuzz_tests_draw_from_this_module():
    import test_gpu_fuzz
    import test_gpu_step_overlap

    assert test_gpu_fuzz.random_states is fs.random_states
    assert test_gpu_step_overlap.fz.random_states is fs.random_states


@pytest.mark.parametrize("variant,na", [("small", 4), ("medium", 1), ("medium", 8), ("large", 16)])
@pytest.mark.parametrize("full", [True, False])
def test_fixed_agent_count(variant, na, full):
    """n_fixed: every env holds `na` agents inside the grid, crowded (envs with agents sharing a cell
    occur wherever na > 1); request counts are R when full and reach below R otherwise."""
    L = oc.layout_for(variant)
    n, pos, atg, tgt, tim, t = fs.random_states(L, 200, na, np.random.RandomState(5), ts=fs.place_ts(L.T), full=full,
                                                n_fixed=na)
    assert (n == na).all() and n.dtype == np.int32
    assert pos.shape == (200, na, 2) and pos.min() >= 0 and pos.max() < L.D
    opened = (tgt >= 0).sum(1)
    np.testing.assert_array_equal(opened, (tim > 0).sum(1))
    assert opened.max() == L.R and (opened.min() == L.R if full else opened.min() < L.R)
    # three requests in ten are at timer 1, of at least R / 2 >= 2 on average: 120 expected or more
    assert tim.max() <= L.W and (tim == 1).sum() >= 30
    assert set(np.unique(t)) == set(fs.place_ts(L.T))
    assert atg.max() < L.Dp and (atg >= 0).any() and (atg < 0).any()
    if na > 1:
        cells = pos[:, :, 0] * L.D + pos[:, :, 1]
        assert any(len(np.unique(c)) < na for c in cells)


def test_canonical_and_bstate_are_one_draw():
    L = oc.layout_for("medium")
    st = fs.random_states(L, 9, 9, np.random.RandomState(3))
    c, S = fs.canonical(*st), fs.bstate(*st)
    for key, field in (("pos", "pos"), ("agent_target", "agent_tgt"), ("pickup_target", "pk_tgt"),
                       ("pickup_timer", "pk_timer"), ("t", "t"), ("n", "n")):
        np.testing.assert_array_equal(c[key], getattr(S, field))
        assert not np.shares_memory(c[key], getattr(S, field))
    assert not S.fresh.any() and not S.episode.any() and S.t.dtype == np.int64


@pytest.mark.parametrize("variant,na,train", [("medium", 8, False), ("medium", None, True)])
def test_place_fuzzed_on_the_host_engine(variant, na, train):
    """The env holds the draw (to_canonical gives it back), fixed-count envs with n == agent_slots,
    Train envs with drawn counts; the same seed gives the same state."""
    import warehouse
    from wide_cases import assert_same, canon

    envs = [warehouse.BatchedWarehouse(variant, 60, na, train=train, seed=1, device="cpu") for _ in range(2)]
    st = fs.place_fuzzed(envs[0], True, 77)
    fs.place_fuzzed(envs[1], True, 77)
    assert_same(canon(envs[0]), fs.bstate(*st))
    assert bool((envs[0].state == envs[1].state).all())
    assert len(set(st[0].tolist())) > 1 if train else (st[0] == na).all()
