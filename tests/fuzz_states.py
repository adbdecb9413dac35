"""Adversarial env states for the fuzz tests (the G2 recipe): agents crowded on a few cells, on
pickup blocks, hugging delivery cells, overlapping; request timers about to expire; clocks at chosen
values.  Such states are not all reachable by an episode (a request opened at t0 >= 0 lives W steps,
so none is about to expire at t = 5): a kernel that assumes reachability is what they are for.

random_states is the generator test_gpu_fuzz.py, test_gpu_step_overlap.py and wide_cases.case_fuzz
have always drawn from; its RNG call order is pinned by tests/test_fuzz_states_cpu.py.  canonical /
bstate turn one draw into the `from_canonical` dict and the oracle's BState; place_fuzzed puts an env
into one draw (the replay and record cases start from it).
"""
import numpy as np

from oracle import batched as ob
from oracle import core as oc


def random_states(L, B, nmax, rng, ts=None, full=False, n_fixed=None):
    """One draw: (n, pos, agent_target, pickup_target, pickup_timer, t) of B envs with nmax agent
    slots.  `full` opens exactly R requests per env (what every reachable pre-step state holds and the
    greedy walk requires), otherwise between max(0, R - n) and R.  `n_fixed` gives every env that many
    agents (a fixed-count env holds n == agent_slots) instead of drawing n ~ U{1..nmax}; the agents are
    crowded by the same four placement modes."""
    P, Dp, R, W, D = L.P, L.Dp, L.R, L.W, L.D
    pk, dl, _, _ = ob.tables(L)
    n = rng.randint(1, nmax + 1, size=B) if n_fixed is None else np.full(B, n_fixed)
    pos = np.zeros((B, nmax, 2), np.int32)
    atg = np.full((B, nmax), -1, np.int32)
    tgt = np.full((B, P), -1, np.int32)
    tim = np.full((B, P), -1, np.int32)
    t = rng.choice(ts if ts is not None else [0, 5, L.T - 1, L.T, 150], size=B).astype(np.int64)
    for e in range(B):
        k = n[e]
        mode = rng.randint(4)
        if mode == 0:
            cx, cy = rng.randint(0, D - 2, size=2)
            p = np.stack([cx + rng.randint(0, 3, k), cy + rng.randint(0, 3, k)], 1)
        elif mode == 1:
            c = pk[rng.randint(P)]
            p = np.stack([c[0] + rng.randint(-1, 2, k), c[1] + rng.randint(-1, 2, k)], 1)
        elif mode == 2:
            c = dl[rng.randint(Dp)]
            p = np.stack([c[0] + rng.randint(-1, 2, k), c[1] + rng.randint(-1, 2, k)], 1)
        else:
            p = rng.randint(0, D, size=(k, 2))
        pos[e, :k] = np.clip(p, 0, D - 1)
        na = R if full else rng.randint(max(0, R - k), R + 1)
        sel = rng.choice(P, na, replace=False)
        tgt[e, sel] = rng.randint(0, Dp, na)
        tim[e, sel] = np.where(rng.rand(na) < 0.3, 1, rng.randint(1, W + 1, na))
        a = np.where(rng.rand(k) < 0.4, rng.randint(0, Dp, k), -1)
        for i in range(k):
            if a[i] >= 0 and rng.rand() < 0.5:
                pos[e, i] = np.clip(dl[a[i]] + rng.randint(-1, 2, 2), 0, D - 1)
        atg[e, :k] = a
    return n.astype(np.int32), pos, atg, tgt, tim, t


def canonical(n, pos, atg, tgt, tim, t):
    """The `from_canonical` dict of one draw (fresh = 0, episode = 0)."""
    return dict(pos=pos, agent_target=atg, pickup_target=tgt, pickup_timer=tim, t=t, n=n)


def bstate(n, pos, atg, tgt, tim, t):
    """The oracle's BState of one draw (its own copies)."""
    B = len(n)
    return ob.BState(pos=pos.copy(), agent_tgt=atg.copy(), pk_tgt=tgt.copy(), pk_timer=tim.copy(), t=t.copy(),
                     n=n.copy(), fresh=np.zeros(B, bool), episode=np.zeros(B, np.uint32))


def place_ts(T):
    """place_fuzzed's clocks: far below W (where no episode holds a request about to expire), mid
    episode, and the last three steps and the end of one."""
    return [0, 5, 57, 150, T - 3, T - 2, T - 1, T]


def draw_for(env, full, seed):
    """The draw place_fuzzed puts `env` into: agent_slots slots, every env holding agent_slots agents
    unless the env is a Train one (n drawn), clocks from place_ts."""
    L = oc.layout_for(env.variant)
    return random_states(L, env.B, env.agent_slots, np.random.RandomState(seed), ts=place_ts(L.T), full=full,
                         n_fixed=None if env.train else env.agent_slots)


def place_fuzzed(env, full, seed):
    """env.reset(), then the env into one draw.  full=True: R open requests everywhere, as the greedy
    walk requires; full=False: sparse request tables, for external actions only.  Returns the draw."""
    env.reset()
    st = draw_for(env, full, seed)
    env.from_canonical(canonical(*st))
    return st
