"""Test bodies of the 16-lanes-per-env step form, each taking an env factory
`make(variant, num_envs, num_agents, **kw) -> BatchedWarehouse`.

tests/test_gpu_wide.py runs them with lanes_per_env=16 on the GPU; tests/test_wide_cpu.py runs the
same bodies on the host engine (lanes_per_env=1), which checks the inputs and the oracle against
each other before any GPU time is spent.  Every comparison is bit-exact, against the
reference-generated fixtures under tests/golden or the fixture-pinned oracle.
"""
import glob
import os

import numpy as np
import torch

from oracle import batched as ob
from oracle import core as oc

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FIELDS = ("pos", "agent_tgt", "pk_tgt", "pk_timer", "t", "n", "fresh", "episode")

# (variant, agents, train, policy, p, staggered)
ROLLOUT_SHAPES = [("small", 4, False, "random", 0.0, False), ("medium", 8, False, "greedy", 0.0, True),
                  ("large", 16, False, "greedy", 0.05, False), ("medium", 9, True, "greedy", 0.3, False),
                  ("large", 7, False, "greedy", 0.0, False)]
CO_LOCATED_SHAPES = [("medium", 8, "greedy", 0.25), ("small", 4, "random", 0.0)]


def canon(env):
    return {k: v.cpu().numpy() for k, v in env.to_canonical().items()}


def oracle_state(c):
    return ob.BState(pos=c["pos"].copy(), agent_tgt=c["agent_target"].copy(), pk_tgt=c["pickup_target"].copy(),
                     pk_timer=c["pickup_timer"].copy(), t=c["t"].astype(np.int64), n=c["n"].copy(),
                     fresh=c["fresh"].astype(bool), episode=c["episode"].astype(np.uint32))


def assert_same(c, S, msg=""):
    np.testing.assert_array_equal(c["pos"], S.pos, err_msg=msg)
    np.testing.assert_array_equal(c["agent_target"], S.agent_tgt, err_msg=msg)
    np.testing.assert_array_equal(c["pickup_target"], S.pk_tgt, err_msg=msg)
    np.testing.assert_array_equal(c["pickup_timer"], S.pk_timer, err_msg=msg)
    np.testing.assert_array_equal(c["t"], S.t, err_msg=msg)
    np.testing.assert_array_equal(c["n"], S.n, err_msg=msg)
    np.testing.assert_array_equal(c["fresh"].astype(bool), S.fresh, err_msg=msg)
    np.testing.assert_array_equal(c["episode"].astype(np.uint32), S.episode, err_msg=msg)


def take(S, idx):
    return ob.BState(*(getattr(S, f)[idx].copy() for f in FIELDS))


def put(S, idx, sub):
    for f in FIELDS:
        getattr(S, f)[idx] = getattr(sub, f)


class Bins:
    """Oracle of wh_episode_stats: on_episode_end (scripts/train.py:18-23) binned by n."""

    def __init__(self, na):
        self.sum = np.zeros(na + 1, np.int64)
        self.cnt = np.zeros(na + 1, np.int64)
        self.mn = np.full(na + 1, 0xFFFFFFFF, np.int64)
        self.mx = np.zeros(na + 1, np.int64)

    def fold(self, ret, n, done):
        for e in np.flatnonzero(done):
            b, r = int(n[e]), int(ret[e])
            self.sum[b] += r
            self.cnt[b] += 1
            self.mn[b] = min(self.mn[b], r)
            self.mx[b] = max(self.mx[b], r)

    def check(self, stats):
        got = stats.bins()
        np.testing.assert_array_equal(got["return_sum"], self.sum)
        np.testing.assert_array_equal(got["episodes"], self.cnt)
        np.testing.assert_array_equal(got["return_min"].astype(np.int64), self.mn)
        np.testing.assert_array_equal(got["return_max"].astype(np.int64), self.mx)


# ----------------------------------------------------------------------------- 1. reference episodes
def case_g1_episodes(make, variant):
    """The ascending-order g1_* / ord_* reference episodes of a variant, batched as B = runs: injected
    reset draws, injected regeneration; state, rewards, dones and rows at each of the 200 steps."""
    paths = sorted(glob.glob(os.path.join(GOLDEN, f"g1_{variant}_*.npz"))
                   + glob.glob(os.path.join(GOLDEN, f"ord_{variant}_*.npz")))
    runs = [dict(np.load(p)) for p in paths]
    runs = [g for g in runs if np.all(g["order"] == np.arange(int(g["n"])))]
    assert len(runs) >= 4
    nmax = oc.VARIANTS[variant]["nmax"]
    B = len(runs)
    n = np.array([int(g["n"]) for g in runs], np.int32)
    spawn = np.zeros((B, nmax, 2), np.int32)
    for e, g in enumerate(runs):
        spawn[e, : n[e]] = g["spawn"]
    env = make(variant, B, None, train=True)
    env.reset(draws=dict(spawn=spawn, pickups=np.stack([g["reset_sel"] for g in runs]),
                         targets=np.stack([g["reset_tgt"] for g in runs]), n=n))
    obs = env.observe().cpu().numpy()
    for e, g in enumerate(runs):
        np.testing.assert_array_equal(obs[e, : n[e]], g["reset_obs"])
    for s in range(200):
        acts = np.full((B, nmax), 4, np.int32)
        for e, g in enumerate(runs):
            acts[e, : n[e]] = np.mod(g["actions"][s], 9)
        regen = np.concatenate([np.stack([g["rpos"][s] for g in runs]),
                                np.stack([g["rtgt"][s] for g in runs])], axis=1)
        rew, done = env.step(acts, regen=regen)
        rew, done = rew.cpu().numpy(), done.cpu().numpy()
        c = canon(env)
        obs = env.observe().cpu().numpy()
        for e, g in enumerate(runs):
            k = n[e]
            np.testing.assert_array_equal(c["pos"][e, :k], g["pos"][s], err_msg=f"env {e} step {s}")
            np.testing.assert_array_equal(c["agent_target"][e, :k], g["agent_tgt"][s], err_msg=f"env {e} step {s}")
            np.testing.assert_array_equal(c["pickup_target"][e], g["pk_tgt"][s], err_msg=f"env {e} step {s}")
            np.testing.assert_array_equal(c["pickup_timer"][e], g["pk_timer"][s], err_msg=f"env {e} step {s}")
            assert c["t"][e] == g["t"][s]
            np.testing.assert_array_equal(rew[e, :k], g["rewards"][s], err_msg=f"env {e} step {s}")
            assert not rew[e, k:].any()
            assert bool(done[e]) == bool(g["done"][s])
            np.testing.assert_array_equal(obs[e, :k], g["obs"][s], err_msg=f"env {e} step {s}")


# ----------------------------------------------------------------------------- 2. dense transitions
def case_g2_dense(make, variant):
    """The g2 known-answer transitions whose action-dict order is every live agent, ascending (each
    variant's fixture has more than 200 such rows)."""
    g = np.load(os.path.join(GOLDEN, f"g2_{variant}.npz"))
    n, order = g["n"], g["order"]
    idx = np.array([e for e in range(len(n)) if np.array_equal(order[e, : n[e]], np.arange(n[e]))
                    and (order[e, n[e]:] == -1).all()])
    assert len(idx) > 200
    env = make(variant, len(idx), None, train=True)
    env.from_canonical(dict(pos=g["pre_pos"][idx], agent_target=g["pre_agent_tgt"][idx],
                            pickup_target=g["pre_pk_tgt"][idx], pickup_timer=g["pre_pk_timer"][idx],
                            t=g["pre_t"][idx], n=n[idx]))
    regen = np.concatenate([g["rpos"], g["rtgt"]], axis=1)[idx]
    rew, done = env.step(g["actions"][idx], regen=regen)
    c = canon(env)
    np.testing.assert_array_equal(c["pos"], g["pos"][idx])
    np.testing.assert_array_equal(c["agent_target"], g["agent_tgt"][idx])
    np.testing.assert_array_equal(c["pickup_target"], g["pk_tgt"][idx])
    np.testing.assert_array_equal(c["pickup_timer"], g["pk_timer"][idx])
    np.testing.assert_array_equal(rew.cpu().numpy(), g["rewards"][idx])
    np.testing.assert_array_equal(done.cpu().numpy().astype(bool), g["done"][idx])
    np.testing.assert_array_equal(env.observe().cpu().numpy(), g["obs"][idx])
    if env.lanes_per_env != 1:   # the wide step reports |inactive| although it runs the whole step
        np.testing.assert_array_equal(env.n_inactive.cpu().numpy(), g["n_inactive"][idx])


# ----------------------------------------------------------------------------- 3. fuzzed transitions
def case_fuzz(make, variant, B=1237, seed=41):
    """One philox-regenerated step from adversarial states (crowded, overlapping agents, timers about
    to expire, t in {0, 5, 150, T-1, T}); B is odd: a partial last group, wave and workgroup; Train
    slots, so n < slots leaves idle lanes."""
    from fuzz_states import random_states

    L = oc.layout_for(variant)
    nmax = oc.VARIANTS[variant]["nmax"]
    rng = np.random.RandomState(900 + nmax)
    n, pos, atg, tgt, tim, t = random_states(L, B, nmax, rng)
    env = make(variant, B, None, train=True, seed=seed)
    env.from_canonical(dict(pos=pos, agent_target=atg, pickup_target=tgt, pickup_timer=tim, t=t, n=n))
    S = ob.BState(pos=pos.copy(), agent_tgt=atg.copy(), pk_tgt=tgt.copy(), pk_timer=tim.copy(), t=t.copy(),
                  n=n.copy(), fresh=np.zeros(B, bool), episode=np.zeros(B, np.uint32))
    acts = rng.randint(0, 9, size=(B, nmax)).astype(np.int32)
    rew, done = env.step(acts)
    orew, odone, on_in, _ = ob.step(L, S, acts, ob.PhiloxDraws(seed, np.arange(B)))
    assert_same(canon(env), S)
    np.testing.assert_array_equal(rew.cpu().numpy(), orew)
    np.testing.assert_array_equal(done.cpu().numpy().astype(bool), odone)
    np.testing.assert_array_equal(env.observe().cpu().numpy(), ob.observe(L, S))
    if env.lanes_per_env != 1:
        np.testing.assert_array_equal(env.n_inactive.cpu().numpy(), on_in)


# ----------------------------------------------------------------------------- 4. fused rollouts
def oracle_rollout(L, S, d, K, policy, p, nmax, rew, dn, bins=None, epret=None):
    """K oracle iterations of {policy, step, auto-reset} checked against per-step rewards / dones;
    returns the summed rewards per env."""
    tot = np.zeros(S.B, np.float32)
    for s in range(K):
        acts = ob.greedy(L, S, p, d) if policy == "greedy" else ob.random_actions(S, d)
        orew, odone, _, _ = ob.step(L, S, acts, d)
        np.testing.assert_array_equal(rew[s], orew, err_msg=f"step {s}")
        np.testing.assert_array_equal(dn[s].astype(bool), odone, err_msg=f"step {s}")
        tot += orew.sum(1)
        if bins is not None:
            epret += orew.sum(1).astype(np.int64)
            bins.fold(epret, S.n, odone)
            epret[odone] = 0
        if odone.any():
            ob.reset(L, S, d, mask=odone, nmax=nmax)
    return tot


def case_fused_rollout(make, variant, na, train, policy, p, staggered, B=83, K=230, seed=3):
    """wh_rollout's recipe (K steps in one launch across an episode end, in-kernel auto-reset, Train
    variants redrawing n) with rewards, dones, returns and episode metrics, against the oracle; when
    `staggered`, from clocks offset by (37 e) mod 200 so that envs of one wave end on different steps."""
    L = oc.layout_for(variant)
    nmax = na if train else None
    env = make(variant, B, None if train else na, train=train, seed=seed)
    env.reset()
    ids = np.arange(B)
    d = ob.PhiloxDraws(seed, ids)
    S = ob.BState.zeros(L, B, na)
    ob.reset(L, S, d, nmax=nmax)
    if staggered:
        off = (37 * ids) % 200
        env.stagger(off)
        for s in range(int(off.max())):
            idx = np.flatnonzero(off > s)
            sub = take(S, idx)
            ds = ob.PhiloxDraws(seed, idx)
            _, odone, _, _ = ob.step(L, sub, ob.greedy(L, sub, 0.0, ds), ds)
            if odone.any():
                ob.reset(L, sub, ds, mask=odone, nmax=nmax)
            put(S, idx, sub)
        assert len(np.unique(S.t)) > 40
        assert_same(canon(env), S, "after stagger")
    st = env.enable_episode_stats()
    rew = torch.zeros((K, B, na), device=env.device)
    dn = torch.zeros((K, B), dtype=torch.uint8, device=env.device)
    ret = torch.full((B,), 2.0, device=env.device)   # returns are accumulated (+=)
    env.rollout(K, policy, p, rewards=rew, dones=dn, returns=ret)
    bins, epret = Bins(na), np.zeros(B, np.int64)
    tot = oracle_rollout(L, S, d, K, policy, p, nmax, rew.cpu().numpy(), dn.cpu().numpy(), bins, epret)
    assert dn.sum().item() >= B                      # every env crossed an episode end
    assert_same(canon(env), S, "after rollout")
    np.testing.assert_array_equal(ret.cpu().numpy(), tot + 2.0)
    bins.check(st)
    np.testing.assert_array_equal(st.episode_return.cpu().numpy(), epret)
    np.testing.assert_array_equal(env.observe().cpu().numpy(), ob.observe(L, S))


# ----------------------------------------------------------------------------- 5. co-located agents
def case_co_located(make, variant, na, policy, p, B=83, K=230, seed=17):
    """Agents sharing cells: one leaving clears the cell under the one that stays (core.py:289-291)
    until the next step's rebuild (core.py:275-276)."""
    L = oc.layout_for(variant)
    env = make(variant, B, na, seed=seed)
    env.reset()
    env.rollout(13, "greedy", 0.0)
    c = canon(env)
    rng = np.random.RandomState(1)
    pos = c["pos"].copy()
    for e in range(B):
        k = rng.randint(1, na // 2 + 1)                         # k pairs share a cell
        slots = rng.permutation(na)[: 2 * k]
        pos[e, slots[1::2]] = pos[e, slots[0::2]]
    c["pos"] = pos
    env.from_canonical(c)
    S = oracle_state(canon(env))
    rew = torch.zeros((K, B, na), device=env.device)
    dn = torch.zeros((K, B), dtype=torch.uint8, device=env.device)
    env.rollout(K, policy, p, rewards=rew, dones=dn)
    d = ob.PhiloxDraws(seed, np.arange(B))
    oracle_rollout(L, S, d, K, policy, p, None, rew.cpu().numpy(), dn.cpu().numpy())
    assert_same(canon(env), S, "after rollout")


# ----------------------------------------------------------------------------- 6. vector_step
def case_vector_step(make, B=19, K=30, seed=21):
    """wh_vector_step's recipe at Medium (Train, 9 slots): a random env mask, external actions,
    auto-reset with n redrawn, rows every step, episode metrics.  Clocks start at 185..192 so that
    envs end inside the 30 steps.  Masked-out envs keep their state and their stale rewards / dones;
    the rows of a done env are the first rows of its next episode."""
    variant, na = "medium", 9
    L = oc.layout_for(variant)
    env = make(variant, B, None, train=True, seed=seed)
    env.reset()
    c = canon(env)
    c["t"] = (185 + np.arange(B) % 8).astype(np.int32)
    c["fresh"] = np.zeros(B, bool)
    env.from_canonical(c)
    S = oracle_state(canon(env))
    st = env.enable_episode_stats()
    bins, epret = Bins(na), np.zeros(B, np.int64)
    rng = np.random.RandomState(2)
    prev_rew, prev_done = np.zeros((B, na), np.float32), np.zeros(B, np.uint8)
    ends = 0
    for s in range(K):
        acts = rng.randint(0, 9, size=(B, na)).astype(np.int32)
        m = rng.rand(B) < 0.6
        obs, rew, done = env.vector_step(acts, autoreset=True, observe=True, mask=m)
        rew, done = rew.cpu().numpy().copy(), done.cpu().numpy().copy()
        idx = np.flatnonzero(m)
        sub = take(S, idx)
        d = ob.PhiloxDraws(seed, idx)
        orew, odone, _, _ = ob.step(L, sub, acts[idx], d)
        np.testing.assert_array_equal(rew[idx], orew, err_msg=f"step {s}")
        np.testing.assert_array_equal(done[idx].astype(bool), odone, err_msg=f"step {s}")
        np.testing.assert_array_equal(rew[~m], prev_rew[~m], err_msg=f"stale rewards, step {s}")
        np.testing.assert_array_equal(done[~m], prev_done[~m], err_msg=f"stale dones, step {s}")
        prev_rew, prev_done = rew, done
        epret[idx] += orew.sum(1).astype(np.int64)
        full_done = np.zeros(B, bool)
        full_done[idx] = odone
        bins.fold(epret, S.n, full_done)
        epret[full_done] = 0
        ends += int(odone.sum())
        if odone.any():
            ob.reset(L, sub, d, mask=odone, nmax=na)
        put(S, idx, sub)
        assert_same(canon(env), S, f"step {s}")
        np.testing.assert_array_equal(obs.cpu().numpy(), ob.observe(L, S), err_msg=f"rows, step {s}")
    assert ends >= 10
    bins.check(st)
    np.testing.assert_array_equal(st.episode_return.cpu().numpy(), epret)


# ----------------------------------------------------------------------------- 7. shard invariance
def case_shards(make, K=210, seed=11):
    """One batch of 40 Medium-8 envs == shards of 23 and 17 at env_offset 0 and 23, and both == oracle."""
    variant, na, B = "medium", 8, 40
    L = oc.layout_for(variant)

    def run(b, off):
        env = make(variant, b, na, seed=seed, env_offset=off)
        env.reset()
        rew = torch.zeros((K, b, na), device=env.device)
        dn = torch.zeros((K, b), dtype=torch.uint8, device=env.device)
        env.rollout(K, "greedy", 0.0, rewards=rew, dones=dn)
        return env, rew.cpu().numpy(), dn.cpu().numpy()

    full, frew, fdn = run(B, 0)
    parts = [run(23, 0), run(17, 23)]
    np.testing.assert_array_equal(np.concatenate([p[1] for p in parts], axis=1), frew)
    np.testing.assert_array_equal(np.concatenate([p[2] for p in parts], axis=1), fdn)
    assert torch.equal(torch.cat([p[0].state for p in parts], dim=1), full.state)
    for (env, rew, dn), ids in zip(parts, (np.arange(23), np.arange(23, 40))):
        S = ob.BState.zeros(L, len(ids), na)
        d = ob.PhiloxDraws(seed, ids)
        ob.reset(L, S, d)
        oracle_rollout(L, S, d, K, "greedy", 0.0, None, rew, dn)
        assert_same(canon(env), S, "shard")


# ----------------------------------------------------------------------------- 8. edges
def case_edges(make, seed=29):
    """B = 1, 3 and 17 (less than a wave, a partial wave, more than a workgroup); n = 1 on Large-16;
    steps = 0 leaves the state untouched."""
    for variant, na, B in (("medium", 8, 1), ("small", 4, 3), ("large", 16, 17)):
        L = oc.layout_for(variant)
        env = make(variant, B, na, seed=seed)
        env.reset()
        K = 25
        rew = torch.zeros((K, B, na), device=env.device)
        dn = torch.zeros((K, B), dtype=torch.uint8, device=env.device)
        env.rollout(K, "greedy", 0.1, rewards=rew, dones=dn)
        S = ob.BState.zeros(L, B, na)
        d = ob.PhiloxDraws(seed, np.arange(B))
        ob.reset(L, S, d)
        oracle_rollout(L, S, d, K, "greedy", 0.1, None, rew.cpu().numpy(), dn.cpu().numpy())
        assert_same(canon(env), S, f"{variant} B={B}")
        before = env.state.clone()
        env.rollout(0, "greedy", 0.0)
        assert torch.equal(env.state, before)
    # one live agent in 16 slots
    L = oc.layout_for("large")
    B, K = 5, 40
    env = make("large", B, None, train=True, seed=seed)
    env.reset()
    c = canon(env)
    c["n"] = np.ones(B, np.int32)
    env.from_canonical(c)
    S = oracle_state(canon(env))
    assert (S.n == 1).all()
    rew = torch.zeros((K, B, 16), device=env.device)
    dn = torch.zeros((K, B), dtype=torch.uint8, device=env.device)
    env.rollout(K, "greedy", 0.0, rewards=rew, dones=dn, autoreset=False)
    d = ob.PhiloxDraws(seed, np.arange(B))
    oracle_rollout(L, S, d, K, "greedy", 0.0, 16, rew.cpu().numpy(), dn.cpu().numpy())
    assert_same(canon(env), S, "n = 1")
    assert rew.sum().item() > 0
