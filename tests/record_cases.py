"""Test bodies of the recorded step (wh_replay_record, k_step_record; ReplayBuffer(fused=...),
ReplayBuffer.collect, warehouse.policy_collect), each taking an env factory as replay_cases.py does.

tests/test_gpu_record.py runs them on the GPU, tests/test_record_cpu.py on the host engine.  The
feature is defined as bit-equality with the five-launch route (put, step without auto-reset, put,
reset, observe), which the oracle already pins, so every comparison is at tolerance 0.  Shapes:
B = 300 -- one full workgroup of 256 envs and one of 44, so records past env 256 and lanes past B are
both exercised -- and B = 37 for one variant; capacity 5 and 9 recorded steps, so the ring wraps; envs
placed at T-3, T-2, T-1 and T-8, so every env ends an episode within the 9 steps.  The *_fuzzed cases
start from fuzz_states.place_fuzzed (requests about to expire at any t, sparse tables, clocks from 0
to T) and hold collect to the oracle's rollout as well; their clocks make envs end an episode early
in a multi-step launch, so the launch goes on stepping envs it has reset itself.
"""
import ctypes

import numpy as np
import torch

import replay_cases as rc
from fuzz_states import bstate, canonical, draw_for, place_fuzzed
from oracle import batched as ob
from oracle import core as oc
from replay_cases import CAP, GUARD, SEED, STEPS, place_near_end
from wide_cases import Bins, assert_same as assert_oracle_state, canon, oracle_rollout

NB = 300
RING = ("states", "actions", "rewards", "dones")


def guard_ring(buf):
    """Move the ring's four tensors into storage followed by GUARD sentinel bytes each."""
    from warehouse import _native as nat

    raw = {}
    for name in RING:
        t = getattr(buf, name)
        nbytes = t.numel() * t.element_size()
        raw[name] = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=t.device)
        v = raw[name][:nbytes].view(t.dtype).reshape(t.shape)
        v.zero_()
        setattr(buf, name, v)
    buf._ring = nat.WhReplayRing(buf.states.data_ptr(), buf.actions.data_ptr(), buf.rewards.data_ptr(),
                                 buf.dones.data_ptr(), buf.capacity)
    return raw


def twins(make, variant, nb, na, train, place=None, **fused):
    """Two envs with one seed and one state, each with episode stats and a guarded buffer: the first
    recorded by the record launch, the second by the five launches.  `place(env)` puts a fresh env
    into its first state (default place_near_end)."""
    import warehouse

    envs = [make(variant, nb, na, train=train, seed=SEED) for _ in range(2)]
    for e in envs:
        (place or place_near_end)(e)
        e.enable_episode_stats()
    assert torch.equal(envs[0].state.cpu(), envs[1].state.cpu())
    bufs = [warehouse.ReplayBuffer(envs[0], CAP, fused=True, **fused),
            warehouse.ReplayBuffer(envs[1], CAP, fused=False, **fused)]
    return envs, bufs, [guard_ring(b) for b in bufs]


def assert_same(envs, bufs, raws, msg):
    """Ring, live state, stats, cursor and filled of the two routes, and the guards of both rings."""
    for name in RING:
        a, b = getattr(bufs[0], name).cpu(), getattr(bufs[1], name).cpu()
        assert torch.equal(a, b), f"{msg}: ring {name} differs"
    assert torch.equal(envs[0].state.cpu(), envs[1].state.cpu()), f"{msg}: live state differs"
    ba, bb = envs[0].stats.bins(), envs[1].stats.bins()
    for k in ba:
        np.testing.assert_array_equal(ba[k], bb[k], err_msg=f"{msg}: stats {k}")
    assert torch.equal(envs[0].stats.episode_return.cpu(), envs[1].stats.episode_return.cpu()), f"{msg}: episode_return"
    assert (bufs[0].cursor, bufs[0].filled) == (bufs[1].cursor, bufs[1].filled), msg
    for raw in raws:
        rc.assert_guards(raw)


# ----------------------------------------------------------------------------- 1. ring equality
def case_ring_equal(make, variant, na, train, nb=NB):
    """step(fused=True) against step(fused=False), after every one of 9 steps: the four ring tensors
    byte for byte, the live state, rows, rewards, dones, stats, cursor and filled."""
    envs, bufs, raws = twins(make, variant, nb, na, train)
    crossed = np.zeros(nb, bool)
    n_seen = set()
    for s in range(STEPS):
        acts = envs[1].policy("greedy", 0.3).clone()
        if s == 2:
            acts[0, 0], acts[nb - 1, -1] = 11, -3   # outside 0 .. 8: recorded (and stepped) as 4
        a, b = bufs[0].step(acts), bufs[1].step(acts)
        assert bufs[0].last_fused is True and bufs[1].last_fused is False
        for x, y, what in zip(a, b, ("obs", "rewards", "dones")):
            assert torch.equal(x.cpu(), y.cpu()), f"{what} differ at step {s}"
        assert_same(envs, bufs, raws, f"{variant}/{na} step {s}")
        assert bufs[0].cursor == (s + 1) % CAP and bufs[0].filled == min(s + 1, CAP)
        if s == 2:
            assert int(bufs[0].actions[2, 0, 0]) == 4 and int(bufs[0].actions[2, nb - 1, -1]) == 4
        crossed |= b[2].cpu().numpy().astype(bool)
        n_seen |= {int(n) for n in canon(envs[1])["n"]}
    assert crossed.all()                                         # every env crossed an episode end
    assert int(envs[0].stats.bins()["episodes"].sum()) >= nb
    if train:
        assert len(n_seen) > 1


# ----------------------------------------------------------------------------- 1b. ring equality, fuzzed
RING_FUZZ_SEED, COLLECT_FUZZ_SEED = 211, 223   # place_fuzzed draws of the two fuzzed cases below


def case_ring_equal_fuzzed(make, variant, na, train, full, nb=NB):
    """case_ring_equal from fuzz_states.place_fuzzed: 9 steps of step(fused=True) against
    step(fused=False), everything equal after every step.  full=True: greedy 0.3 actions; full=False:
    sparse request tables and seeded uniform actions.  Requests must expire inside recorded steps
    (also at t < W, where no episode holds one about to) and envs must be stepped again after a done."""
    envs, bufs, raws = twins(make, variant, nb, na, train, place=lambda e: place_fuzzed(e, full, RING_FUZZ_SEED))
    rng = np.random.default_rng(RING_FUZZ_SEED)
    R, W = envs[0].R, envs[0].geometry["W"]
    was_done = np.zeros(nb, bool)
    cov = dict(expired=0, expired_below_w=0, again=0, sparse=0)
    for s in range(STEPS):
        pre = canon(envs[1])
        if full:
            acts = envs[1].policy("greedy", 0.3).clone()
        else:
            acts = torch.as_tensor(rng.integers(0, 9, (nb, envs[1].agent_slots)).astype(np.int32)).to(envs[1].device)
        a, b = bufs[0].step(acts), bufs[1].step(acts)
        assert bufs[0].last_fused is True and bufs[1].last_fused is False
        for x, y, what in zip(a, b, ("obs", "rewards", "dones")):
            assert torch.equal(x.cpu(), y.cpu()), f"{what} differ at step {s}"
        assert_same(envs, bufs, raws, f"{variant}/{na} full={full} step {s}")
        opened = pre["pickup_target"] >= 0
        last = opened & (pre["pickup_timer"] == 1)            # expiry comes before the pickups: all of them go
        cov["expired"] += int(last.sum())
        cov["expired_below_w"] += int((last & (pre["t"] < W - 1)[:, None]).sum())
        cov["sparse"] += int((opened.sum(1) < R).sum())
        cov["again"] += int(was_done.sum())
        was_done |= b[2].cpu().numpy().astype(bool)
    print(f"coverage {variant}/{na} train={train} full={full}: {cov}")
    assert cov["expired"] >= 1 and cov["expired_below_w"] >= 1 and cov["again"] >= 1, cov
    assert (cov["sparse"] == 0) if full else (cov["sparse"] >= 1), cov
    return cov


# ----------------------------------------------------------------------------- 2. collect
def case_collect_equal(make, variant, na, train, policy, p, prioritized=False, place=None):
    """collect(K, policy, p) against K x [env.policy -> five-launch step], K = 1, 3 and 5 (= capacity)
    from cursor 3, so that K = 3 and K = 5 wrap: returned rows, rewards [K,B,NA], dones [K,B], ring,
    state, stats; with `prioritized`, the tree's leaves, sums and max_q.  Returns the dones [K,B] of
    the K = 5 launch."""
    for K in (1, 3, CAP):
        envs, bufs, raws = twins(make, variant, NB, na, train, place=place, prioritized=prioritized)
        for s in range(3):
            acts = envs[1].policy("greedy", 0.3).clone()
            bufs[0].step(acts), bufs[1].step(acts)
        if prioritized:                                          # priorities above 1.0, so max_q has moved
            for b in bufs:
                b.update_priorities(np.arange(0, 2 * NB, 7), np.linspace(0.5, 9.0, len(np.arange(0, 2 * NB, 7))))
        assert bufs[0].cursor == 3
        obs, rew, done = bufs[0].collect(K, policy, p)
        assert bufs[0].last_fused is True
        assert rew.shape == (K, NB, envs[0].agent_slots) and done.shape == (K, NB)
        launch_dones = done.cpu().numpy().astype(bool)
        for k in range(K):
            o, r, d = bufs[1].step(envs[1].policy(policy, p))
            assert torch.equal(rew[k].cpu(), r.cpu()), f"K={K}: rewards of step {k}"
            assert torch.equal(done[k].cpu(), d.cpu()), f"K={K}: dones of step {k}"
        assert torch.equal(obs.cpu(), o.cpu()), f"K={K}: rows of the final state"
        assert_same(envs, bufs, raws, f"{variant}/{na} {policy} K={K}")
        assert bufs[0].cursor == (3 + K) % CAP and bufs[0].filled == min(3 + K, CAP)
        if prioritized:
            for name in ("prio_leaf", "prio_node", "prio_max_q"):
                assert torch.equal(getattr(bufs[0], name).cpu(), getattr(bufs[1], name).cpu()), f"K={K}: {name}"
            assert int(bufs[0].prio_max_q) > 1 << 20
    # the five-launch fallback of collect itself (fused=False), and steps = 0
    obs2, rew2, done2 = bufs[1].collect(2, policy, p)
    assert bufs[1].last_fused is False and rew2.shape[0] == 2
    obs, rew, done = bufs[0].collect(2, policy, p)
    assert torch.equal(rew.cpu(), rew2.cpu()) and torch.equal(done.cpu(), done2.cpu()) and torch.equal(obs.cpu(), obs2.cpu())
    assert_same(envs, bufs, raws, "collect fallback")
    cur = bufs[0].cursor
    assert bufs[0].collect(0, policy, p)[1].shape[0] == 0 and bufs[0].cursor == cur
    return launch_dones


def steps_after_reset(dones):
    """Env-steps of a launch taken after the launch reset that env: dones [K, B] of its steps."""
    d = np.asarray(dones).astype(bool)
    return int((np.cumsum(d, axis=0) - d > 0).sum())


def case_collect_steps_on_after_resets(make):
    """case_collect_equal from clocks T-5, T-4, T-6 and T-9: after the three single steps the envs sit
    at T-2, T-1, T-3 and T-6, so collect(5) resets three quarters of them at its steps 1, 0 and 2 and
    goes on stepping them -- the reachable twin of case_collect_fuzzed's states."""
    lead = (5, 4, 6, 9)
    dones = case_collect_equal(make, "medium", 8, False, "greedy", 0.3, place=lambda e: place_near_end(e, lead=lead))
    for g, first in enumerate((1, 0, 2, None)):
        col = dones[:, g::4]
        assert (col.any(0) == (first is not None)).all()
        if first is not None:
            assert col[first].all() and col.sum() == col.shape[1]
    assert steps_after_reset(dones) == NB // 4 * (3 + 4 + 2)


# ----------------------------------------------------------------------------- 2b. collect, fuzzed
def case_collect_fuzzed(make, variant, na, train, policy, p, prioritized=False):
    """From place_fuzzed(full=True): three single steps (cursor 3), then collect(5, policy, p), against
    5 x [env.policy -> five-launch step] as case_collect_equal does AND against the oracle's rollout
    under the same philox contract: rewards and dones of every step, and at the end the rows, the
    canonical state and the episode-stat bins.  The three single steps take every env placed at
    T-3 .. T across its episode end, so the envs are placed again (a second draw) before the launch:
    its clocks T-3 .. T make the launch reset envs at its steps 2, 1, 0 and 0 and go on stepping them,
    at least 100 such env-steps.  The stats keep running across the second placement."""
    K, drawn = CAP, []
    envs, bufs, raws = twins(make, variant, NB, na, train, prioritized=prioritized,
                             place=lambda e: drawn.append(place_fuzzed(e, True, COLLECT_FUZZ_SEED)))
    L, slots = oc.layout_for(variant), envs[0].agent_slots
    S, d = bstate(*drawn[0]), ob.PhiloxDraws(SEED, np.arange(NB))
    bins, epret = Bins(slots), np.zeros(NB, np.int64)
    nmax = slots if train else None
    rew3, dn3 = np.zeros((3, NB, slots), np.float32), np.zeros((3, NB), bool)
    for s in range(3):
        acts = envs[1].policy("greedy", 0.3).clone()
        bufs[0].step(acts)
        _, r, dn = bufs[1].step(acts)
        rew3[s], dn3[s] = r.cpu().numpy(), dn.cpu().numpy().astype(bool)
    oracle_rollout(L, S, d, 3, "greedy", 0.3, nmax, rew3, dn3, bins, epret)
    assert_oracle_state(canon(envs[0]), S, "after the single steps")
    for e in envs:
        e.from_canonical(canonical(*draw_for(e, True, COLLECT_FUZZ_SEED + 1)))
    S = bstate(*draw_for(envs[0], True, COLLECT_FUZZ_SEED + 1))
    if prioritized:
        for b in bufs:
            b.update_priorities(np.arange(0, 2 * NB, 7), np.linspace(0.5, 9.0, len(np.arange(0, 2 * NB, 7))))
    assert bufs[0].cursor == 3
    obs, rew, done = bufs[0].collect(K, policy, p)
    assert bufs[0].last_fused is True
    for k in range(K):
        o, r, dn = bufs[1].step(envs[1].policy(policy, p))
        assert torch.equal(rew[k].cpu(), r.cpu()), f"rewards of step {k}"
        assert torch.equal(done[k].cpu(), dn.cpu()), f"dones of step {k}"
    assert torch.equal(obs.cpu(), o.cpu()), "rows of the final state"
    assert_same(envs, bufs, raws, f"{variant}/{na} {policy} {p} fuzzed")
    assert bufs[0].cursor == (3 + K) % CAP and bufs[0].filled == CAP
    if prioritized:
        for name in ("prio_leaf", "prio_node", "prio_max_q"):
            assert torch.equal(getattr(bufs[0], name).cpu(), getattr(bufs[1], name).cpu()), name
        assert int(bufs[0].prio_max_q) > 1 << 20
    dones = done.cpu().numpy().astype(bool)
    oracle_rollout(L, S, d, K, policy, p, nmax, rew.cpu().numpy(), dones, bins, epret)
    assert_oracle_state(canon(envs[0]), S, "after collect")
    np.testing.assert_array_equal(obs.cpu().numpy(), ob.observe(L, S))
    bins.check(envs[0].stats)
    np.testing.assert_array_equal(envs[0].stats.episode_return.cpu().numpy(), epret)
    again = steps_after_reset(dones)
    print(f"coverage {variant}/{na} train={train} {policy} {p}: steps after an in-launch reset {again}")
    assert again >= 100, again
    return again


# ----------------------------------------------------------------------------- 3. sample after record
def case_sample_after_record(make, variant, na, train):
    """A ring recorded by the record launch, gathered: replay_cases.Recording.expected -- the oracle's
    rows of the captured states -- for a permutation of every entry, before and after the wrap."""
    import warehouse

    rec = rc.Recording(make, variant, na, train)
    env = make(variant, rc.B, na, train=train, seed=SEED)
    place_near_end(env)
    buf = warehouse.ReplayBuffer(env, CAP, fused=True)
    rng = np.random.default_rng(11)
    stepped = 0
    for upto in (4, STEPS):
        rec.run(upto)
        while stepped < upto:                                    # the same actions from the same state
            buf.step(rec.steps[stepped]["actions"])
            stepped += 1
        assert (buf.cursor, buf.filled) == (rec.buf.cursor, rec.buf.filled) and buf.last_fused is True
        idx = rng.permutation(len(buf))
        got, want = rc.gather(buf, idx), rec.expected(idx)
        rc.assert_batch(got, {k: want[k] for k in got}, f"{variant}/{na} after {upto} steps: ")


# ----------------------------------------------------------------------------- 4. fragments (device)
def case_fragments(make, variant, na):
    """step(operand="fragments") returns the bytes of vector_step_x(autoreset=True), on either
    route; policy_collect leaves the ring, the actions and the state of policy_rollout with a
    recorder that does the five launches by hand."""
    import warehouse

    envs, bufs, raws = twins(make, variant, NB, na, False)
    plain = make(variant, NB, na, seed=SEED)
    place_near_end(plain)
    for s in range(4):
        acts = plain.policy("greedy", 0.3).clone()
        want = plain.vector_step_x(acts, autoreset=True)
        for b in bufs:
            got = b.step(acts, operand="fragments")
            assert got[0] is b.env._xfrag
            for x, y, what in zip(got, want, ("fragments", "rewards", "dones")):
                assert torch.equal(x, y), f"{what} differ at step {s} (fused={b.last_fused})"
        assert_same(envs, bufs, raws, f"fragments step {s}")
    assert bufs[0].step(acts, operand="fragments", observe=False)[0] is None
    bufs[1].step(acts, observe=False)

    policy_collect_equal(make, variant, na, 6)


def policy_collect_equal(make, variant, na, K, place=None):
    """warehouse.policy_collect (bf16 and f32 network) against policy_rollout with a recorder that does
    the five launches by hand: ring, state, stats, returned operand and the ring's actions.  Returns
    the dones [K, B] of the last network's trajectory."""
    import warehouse

    for precision in ("bf16", "f32"):
        net = warehouse.policy.MLPPolicy(variant, seed=21, precision=precision)
        envs, bufs, raws = twins(make, variant, NB, na, False, place=place)
        roll = make(variant, NB, na, seed=SEED)                  # policy_rollout's own env
        (place or place_near_end)(roll)
        roll.enable_episode_stats()
        seen, dones = [], []

        def record(s, acts, rew, done):
            e, b = envs[1], bufs[1]
            b.put_obs(b.cursor, acts)
            e.vector_step(acts, autoreset=False, observe=False)
            b.put_next(b.cursor)
            e.reset(mask=e.dones)
            b.advance()
            assert torch.equal(rew, e.rewards) and torch.equal(done, e.dones)
            seen.append(acts.clone())
            dones.append(done.cpu().numpy().astype(bool))

        last = warehouse.policy.policy_rollout(roll, net, K, explore=True, seed=9, first_step=4, record=record)
        got = warehouse.policy_collect(bufs[0], net, K, explore=True, seed=9, first_step=4)
        assert torch.equal(got, last) and bufs[0].last_fused is True
        assert_same(envs, bufs, raws, f"policy_collect {precision}")
        assert torch.equal(envs[0].state, roll.state)
        for s in range(max(K - CAP, 0), K):                      # the ring's actions are the network's
            assert torch.equal(bufs[0].actions[s % CAP].to(torch.int32), seen[s]), f"actions of step {s}"
    return np.stack(dones)


def case_policy_collect_fuzzed(make, variant, na):
    """policy_collect from place_fuzzed(full=True), K = 5: the ring byte-equal to policy_rollout with
    the five-launch recorder, with envs stepped on after their reset."""
    dones = policy_collect_equal(make, variant, na, CAP, place=lambda e: place_fuzzed(e, True, COLLECT_FUZZ_SEED))
    assert steps_after_reset(dones) >= 100


# ----------------------------------------------------------------------------- 5. refusals
def case_refusals(nat, lib, host: bool):
    """The host-checkable refusals of wh_replay_record: codes of one library, as a list (the caller
    compares the two libraries' lists).  Pointers are dummies that a refused call never dereferences,
    except on the host engine, where they are real sentinel-filled buffers that must stay untouched."""
    cfg = nat.make_config(12, 4, (4, 8), 4, 200, 200)          # small/4: words 14
    Bc, cap, words, na, L = 3, 2, 14, 4, 37
    keep = []

    def mem(nbytes):
        if not host:
            return 4096 * (len(keep) + 1)                       # never dereferenced: refused first
        t = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8)
        keep.append(t)
        return t.data_ptr() + (-t.data_ptr()) % 16

    ring = dict(states=mem(cap * 2 * Bc * words * 4), actions=mem(cap * Bc * na), rewards=mem(cap * Bc * na * 4),
                dones=mem(cap * Bc), capacity=cap)
    state, acts, rew, done, obs = mem(words * Bc * 4), mem(Bc * na * 4), mem(cap * Bc * na * 4), mem(cap * Bc), \
        mem(Bc * na * L * 4)
    stats_mem = mem(64)
    bad_stats = nat.WhEpisodeStats(None, stats_mem, None, None, None)   # bins without episode_return

    def call(B=Bc, state_=state, ring_=ring, slot=0, steps=1, policy=0, p=0.0, a=acts, r=rew, d=done, o=obs, xf=None,
             st=None, cfg_=cfg):
        rp = None if ring_ is None else ctypes.byref(nat.WhReplayRing(**ring_))
        return lib.wh_replay_record(ctypes.byref(cfg_), B, state_, rp, slot, steps, policy, p, a, r, d, o, xf,
                                    None if st is None else ctypes.byref(st), 0, 1, 0, None)

    E, OK = nat.WH_EINVAL, nat.WH_OK
    bad_cfg = nat.make_config(12, 4, (4, 8), 0, 200, 200)
    border = nat.make_config(12, 4, (1, 8), 4, 200, 200)
    table = [
        ("NULL ring", call(ring_=None), E),
        ("capacity 0", call(ring_=dict(ring, capacity=0)), E),
        ("slot -1", call(slot=-1), E),
        ("slot = capacity", call(slot=cap), E),
        ("steps < 0", call(steps=-1, policy=1), E),
        ("steps > capacity", call(steps=cap + 1, policy=1), E),
        ("policy 3", call(policy=3), E),
        ("policy -1", call(policy=-1), E),
        ("external actions, steps 2", call(steps=2), E),
        ("p > 1", call(policy=1, p=1.5), E),
        ("p < 0", call(policy=1, p=-0.1), E),
        ("p NaN", call(policy=1, p=float("nan")), E),
        ("bins without episode_return", call(st=bad_stats), E),
        ("xfrag not 16-byte aligned", call(xf=obs + 4), E),
        ("NULL ring states", call(ring_=dict(ring, states=None)), E),
        ("NULL ring actions", call(ring_=dict(ring, actions=None)), E),
        ("NULL ring rewards", call(ring_=dict(ring, rewards=None)), E),
        ("NULL ring dones", call(ring_=dict(ring, dones=None)), E),
        ("external actions NULL", call(a=None), E),
        ("NULL state", call(state_=None), E),
        ("B < 0", call(B=-1), E),
        ("bad config", call(cfg_=bad_cfg), E),
        ("racks on the border", call(cfg_=border), nat.WH_ENOTSUP),
        ("bad option before bad config", call(policy=3, cfg_=border), E),
        ("bad config for an empty batch", call(B=0, cfg_=bad_cfg), E),
        ("B = 0, garbage pointers", call(B=0, state_=8, ring_=dict(states=8, actions=8, rewards=8, dones=8, capacity=cap),
                                          a=8, r=8, d=8, o=16), OK),
        ("steps = 0, garbage pointers", call(steps=0, policy=2, state_=8,
                                              ring_=dict(states=8, actions=8, rewards=8, dones=8, capacity=cap),
                                              a=8, r=8, d=8, o=16), OK),
        ("steps = 0, no ring arrays", call(steps=0, policy=1, ring_=dict(states=None, actions=None, rewards=None,
                                                                         dones=None, capacity=cap), a=None), OK),
    ]
    for what, rc_, want in table:
        assert rc_ == want, f"{what}: got {rc_}, expected {want}"
    for t in keep:
        assert bool((t == 0xA5).all()), "a refused (or empty) call wrote to a buffer"
    return [(what, rc_) for what, rc_, _ in table]
