"""The fused greedy rollout's hoisted launch constants against the oracle (oracle/batched.py), bit for bit:
the eps = 0 instance beside the eps > 0 one, the live masks carried across the step loop where a reset
redraws n (Train variants), the done rows of a tail wave, and Large-16's sixteen agent turns.

Every case starts from the library's reset state, which must equal the oracle's, with the episode
clocks moved so that episode ends -- and with them the in-kernel resets -- fall inside one short launch.
Rewards are sums of 1.0f terms, dones and the packed state are integers: tolerance 0 throughout.
"""
import numpy as np
import pytest

from oracle import batched as ob
from oracle import core as oc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def wh():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    import warehouse

    return warehouse


def canon(env):
    return {k: v.cpu().numpy() for k, v in env.to_canonical().items()}


def assert_same(c, S, msg=""):
    np.testing.assert_array_equal(c["pos"], S.pos, err_msg=msg)
    np.testing.assert_array_equal(c["agent_target"], S.agent_tgt, err_msg=msg)
    np.testing.assert_array_equal(c["pickup_target"], S.pk_tgt, err_msg=msg)
    np.testing.assert_array_equal(c["pickup_timer"], S.pk_timer, err_msg=msg)
    np.testing.assert_array_equal(c["t"], S.t, err_msg=msg)
    np.testing.assert_array_equal(c["n"], S.n, err_msg=msg)
    np.testing.assert_array_equal(c["fresh"].astype(bool), S.fresh, err_msg=msg)
    np.testing.assert_array_equal(c["episode"].astype(np.uint32), S.episode, err_msg=msg)


def rollout_vs_oracle(wh, variant, na, train, B, K, p, steps_left, seed=11):
    """One fused launch of K greedy steps (rewards + dones written, auto-reset: the fast instance) from
    the reset state with env e's clock at T - steps_left[e], against the oracle stepped from the same
    state.  Returns (rewards, dones, n at the start, n at the end, oracle dones)."""
    import torch

    L = oc.layout_for(variant)
    nmax = na if train else None
    env = wh.BatchedWarehouse(variant, B, None if train else na, train=train, seed=seed)
    assert env.agent_slots == na
    env.reset()
    d = ob.PhiloxDraws(seed, np.arange(B))
    S = ob.BState.zeros(L, B, na)
    ob.reset(L, S, d, nmax=nmax)
    c = canon(env)
    assert_same(c, S, "after reset")
    T = int(env.geometry["T"])
    S.t[:] = T - np.asarray(steps_left)
    c["t"] = S.t.astype(np.int32)
    env.from_canonical(c)
    n0 = S.n.copy()
    rew = torch.zeros((K, B, na), device=env.device)
    dn = torch.zeros((K, B), dtype=torch.uint8, device=env.device)
    env.rollout(K, "greedy", p, rewards=rew, dones=dn)
    rew, dn = rew.cpu().numpy(), dn.cpu().numpy().astype(bool)
    odn = np.zeros((K, B), bool)
    for s in range(K):
        live = np.arange(na)[None, :] < S.n[:, None]
        pos0 = S.pos.copy()
        orew, odone, _, _ = ob.step(L, S, ob.greedy(L, S, p, d), d)
        # only live agents move (the carried live masks are the ones of this episode's n)
        assert np.array_equal(S.pos[~live], pos0[~live])
        np.testing.assert_array_equal(rew[s], orew, err_msg=f"rewards, step {s}")
        np.testing.assert_array_equal(dn[s], odone, err_msg=f"dones, step {s}")
        odn[s] = odone
        if odone.any():
            ob.reset(L, S, d, mask=odone, nmax=nmax)
    assert_same(canon(env), S, "after the launch")
    return rew, dn, n0, S.n.copy(), odn


@pytest.mark.parametrize("p", [0.0, 0.25])
def test_eps_instances_full_group_partial_group_and_reset(wh, p):
    """Medium-8, B = 320: one full 256-lane group and one 64-lane wave, K = 12 with the episode ends of
    a wave spread over steps 1 .. 10; p = 0 takes the eps = 0 instance, p = 0.25 the other."""
    B, K = 320, 12
    _, dn, _, _, _ = rollout_vs_oracle(wh, "medium", 8, False, B, K, p, 1 + np.arange(B) % 10)
    assert dn.sum() == B and dn.any(axis=1).sum() == 10   # every env ended once, on ten different steps


def test_hoisted_n_across_a_reset_that_redraws_it(wh):
    """Small Train (per-episode n), B = 128, every env auto-reset once within 16 steps: envs whose n the
    reset changed move exactly their new live agents afterwards (positions, rewards and state equal
    the oracle's)."""
    B, K = 128, 20
    _, dn, n0, n1, _ = rollout_vs_oracle(wh, "small", 4, True, B, K, 0.0, 1 + np.arange(B) % 16)
    assert dn.sum() == B
    assert (n1 > n0).any() and (n1 < n0).any()   # resets grew and shrank the live set


def test_tail_wave_done_row(wh):
    """Medium-8, B = 65: the second wave has one live lane (env 64); its dones and rewards, and those
    of the full wave beside it, across an episode end at step 4."""
    B, K = 65, 8
    rew, dn, _, _, odn = rollout_vs_oracle(wh, "medium", 8, False, B, K, 0.0, np.full(B, 4))
    assert dn[3].all() and dn.sum() == B
    np.testing.assert_array_equal(dn[:, 64], odn[:, 64])


def test_large16_greedy(wh):
    """Large-16, B = 64, K = 8: sixteen agent turns per step, half of the wave ending its episode."""
    B, K = 64, 8
    _, dn, _, _, _ = rollout_vs_oracle(wh, "large", 16, False, B, K, 0.0, np.where(np.arange(B) % 2, 5, 150))
    assert dn.sum() == B // 2
