"""GPU parity of the fused step's reordered schedule: the pickup tail shares a block with
regeneration item 0 (the shared-cell test sits in the reverse-key branch), and k_step's greedy loop
carries the next step's request walk across its back-edge (redone after every form of reset).  Short fused
launches from the fuzzed dense states of test_gpu_fuzz -- so single steps hold a delivery, a pickup
and a regeneration in one env -- against the oracle stepping the same philox contract, bit-exact:
rewards and dones of every step and the final state.  Shapes are the smallest that reach the code:
B = 320 is four full waves of one block plus a wave of the next, B = 300 ends in a partial wave."""
import numpy as np
import pytest

from oracle import batched as ob
from oracle import core as oc

import test_gpu_fuzz as fz

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def wh():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    import warehouse

    return warehouse


def dense_states(variant, B, na, seed, ts):
    """B fuzzed states with exactly `na` agents and R open requests each (the generator draws the
    agent count; a fixed-count env holds `na`), t drawn from `ts`."""
    L = oc.layout_for(variant)
    rng = np.random.RandomState(seed)
    parts, have = [], 0
    while have < B:
        st = fz.random_states(L, 4 * B, na, rng, ts=ts, full=True)
        keep = st[0] == na
        parts.append([x[keep] for x in st])
        have += int(keep.sum())
    n, pos, atg, tgt, tim, t = (np.concatenate([p[i] for p in parts])[:B] for i in range(6))
    return L, n, pos, atg, tgt, tim, t


def load(env, n, pos, atg, tgt, tim, t):
    env.from_canonical(dict(pos=pos, agent_target=atg, pickup_target=tgt, pickup_timer=tim, t=t, n=n))
    B = len(n)
    return ob.BState(pos=pos.copy(), agent_tgt=atg.copy(), pk_tgt=tgt.copy(), pk_timer=tim.copy(), t=t.copy(),
                     n=n.copy(), fresh=np.zeros(B, bool), episode=np.zeros(B, np.uint32))


def assert_state(env, S, msg):
    c = {k: v.cpu().numpy() for k, v in env.to_canonical().items()}
    for key, want in (("pos", S.pos), ("agent_target", S.agent_tgt), ("pickup_target", S.pk_tgt),
                      ("pickup_timer", S.pk_timer), ("t", S.t), ("fresh", S.fresh), ("episode", S.episode)):
        np.testing.assert_array_equal(c[key].astype(np.int64), np.asarray(want).astype(np.int64), err_msg=f"{msg}: {key}")


def rollout_vs_oracle(wh, variant, na, B, K, policy, seed, t, launches=1):
    """`launches` fused launches of K steps against the oracle; returns per-step event counts."""
    import torch

    L, n, pos, atg, tgt, tim, t0 = dense_states(variant, B, na, seed, [0])
    t = np.broadcast_to(np.asarray(t, np.int64), (B,)).copy()
    env = wh.BatchedWarehouse(variant, B, na, seed=seed)
    S = load(env, n, pos, atg, tgt, tim, t)
    d = ob.PhiloxDraws(seed, np.arange(B))
    seen = dict(pickup=0, delivery=0, both=0, resets=[])
    for launch in range(launches):
        rew = torch.zeros((K, B, na), device=env.device)
        dn = torch.zeros((K, B), dtype=torch.uint8, device=env.device)
        env.rollout(K, policy, 0.0, rewards=rew, dones=dn)
        rew, dn = rew.cpu().numpy(), dn.cpu().numpy().astype(bool)
        for s in range(K):
            had = S.agent_tgt >= 0
            acts = ob.greedy(L, S, 0.0, d) if policy == "greedy" else ob.random_actions(S, d)
            orew, odone, _, _ = ob.step(L, S, acts, d)
            np.testing.assert_array_equal(rew[s], orew, err_msg=f"launch {launch} step {s}")
            np.testing.assert_array_equal(dn[s], odone, err_msg=f"launch {launch} step {s}")
            pk, dl = ((orew > 0) & ~had).any(1), ((orew > 0) & had).any(1)
            seen["pickup"] += int(pk.sum())
            seen["delivery"] += int(dl.sum())
            seen["both"] += int((pk & dl).sum())
            if odone.any():
                seen["resets"].append(odone.copy())
                ob.reset(L, S, d, mask=odone)
        assert_state(env, S, f"after launch {launch}")
    return seen


def test_medium8_dense_steps(wh):
    """Medium-8, B = 320, 12-step launches from dense states: steps in which one env both delivers and
    picks up (and, holding fewer than R requests afterwards, regenerates) must occur."""
    seen = rollout_vs_oracle(wh, "medium", 8, 320, 12, "greedy", 41, 20, launches=2)
    assert seen["pickup"] > 0 and seen["delivery"] > 0 and seen["both"] > 0, seen


def staggered_t(B, T, K):
    """Episode clocks so that, inside a K-step launch, wave 0 resets one lane, wave 1 eight lanes on
    one step, wave 2 every lane, wave 3 twenty lanes on one step and wave 4 lanes on several steps."""
    t = np.full(B, 20, np.int64)
    t[5] = T - 3
    t[64 + 3 * np.arange(8)] = T - 4
    t[128:192] = T - 2
    t[192 + 2 * np.arange(20)] = T - 5
    w4 = np.arange(256, B)
    t[w4[::3]] = T - 1 - (w4[::3] % (K - 2))
    return t


@pytest.mark.parametrize("B", [320, 300])
def test_medium8_across_episode_end(wh, B):
    """The same across an episode end with staggered clocks: resets of 1 lane (reset slot), 8 lanes,
    all 64 lanes of a wave and 20 lanes (the per-lane form; with B = 300 also in a partial wave), each
    followed by further steps of the launch, whose carried request walk must be the reset state's."""
    T = oc.layout_for("medium").T
    seen = rollout_vs_oracle(wh, "medium", 8, B, 12, "greedy", 43, staggered_t(B, T, 12))
    per_wave = {tuple(int(m[w * 64:(w + 1) * 64].sum()) for w in range(4)) for m in seen["resets"]}
    assert {(1, 0, 0, 0), (0, 8, 0, 0), (0, 0, 64, 0), (0, 0, 0, 20)} <= per_wave, per_wave
    assert any(m[256:].any() for m in seen["resets"])


@pytest.mark.parametrize("K", [1, 2])
def test_medium8_short_launches(wh, K):
    """Launches of one and of two steps (the rotated loop's first and last iteration), with lanes
    ending their episode on the first and on the last step: one lane of wave 0 (reset from scratch:
    short launches fill no slots), all of wave 1, ten lanes of wave 2."""
    B, T = 320, oc.layout_for("medium").T
    t = np.full(B, 20, np.int64)
    t[7] = T - 1
    t[64:128] = T - 1
    t[128 + 5 * np.arange(10)] = T - 1
    t[200] = T - K
    t[256 + 2 * np.arange(20)] = T - K
    seen = rollout_vs_oracle(wh, "medium", 8, B, K, "greedy", 47, t, launches=2)
    assert seen["resets"] and seen["resets"][0][7] and seen["resets"][0][64:128].all()


def test_small4_random_policy(wh):
    seen = rollout_vs_oracle(wh, "small", 4, 128, 12, "random", 53, 20)
    assert seen["pickup"] + seen["delivery"] > 0, seen


def test_large16_greedy(wh):
    T = oc.layout_for("large").T
    t = np.full(128, 20, np.int64)
    t[64:128:4] = T - 6
    seen = rollout_vs_oracle(wh, "large", 16, 128, 12, "greedy", 59, t)
    assert seen["pickup"] > 0 and seen["delivery"] > 0 and seen["resets"], seen


def test_sampler_rollout_medium8(wh):
    """wh_sampler_rollout (its fast instance shares step_env's merged pickup tail, not the rotation) of
    3 steps at Medium-8, B = 256, from dense states, against policy + vector_step launches: rows,
    rewards, dones and final state."""
    import torch

    B, K, seed = 256, 3, 61
    L, n, pos, atg, tgt, tim, t = dense_states("medium", B, 8, seed, [20])
    t[10] = L.T - 2            # one lane of a wave, and a whole wave, end inside the launch
    t[64:128] = L.T - 1
    a = wh.BatchedWarehouse("medium", B, 8, seed=seed)
    b = wh.BatchedWarehouse("medium", B, 8, seed=seed)
    load(a, n, pos, atg, tgt, tim, t)
    load(b, n, pos, atg, tgt, tim, t)
    obs, rew, dn = a.sampler_rollout(K, "greedy", 0.0)
    for s in range(K):
        ob_, rb, db = b.vector_step(b.policy("greedy", 0.0))
        assert torch.equal(rew[s], rb) and torch.equal(dn[s], db), f"step {s}"
        assert torch.equal(obs[s], ob_), f"obs step {s}"
    assert torch.equal(a.state, b.state)
    assert dn.any()
