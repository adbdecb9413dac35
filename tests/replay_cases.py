"""Test bodies of the replay ring (warehouse.ReplayBuffer, wh_replay_put / wh_replay_gather), each
taking an env factory `make(variant, num_envs, num_agents, **kw) -> BatchedWarehouse`.

tests/test_gpu_replay.py runs them on the GPU; tests/test_replay_cpu.py runs the same bodies on the
host engine.  Every comparison is at tolerance 0: rows are byte values as floats, everything else is
integer or copied.  Shapes throughout: B = 37 envs (no multiple of a workgroup's 4 / 16 / 64 samples,
of a wave or of the put kernel's 256 envs), capacity 5, 9 recorded steps, so the ring wraps.  Envs
start at t = T-3 .. T-1 (and a fourth group at T-8), so different envs end their episode at
different recorded steps, before and after the wrap.  The *_fuzzed cases start from
fuzz_states.place_fuzzed instead: request timers anywhere in 1 .. W (three in ten at 1, also at
t < W), sparse request tables, crowded agents, clocks at 0, 5, 57, 150 and T-3 .. T.
"""
import ctypes

import numpy as np
import torch

from oracle import batched as ob
from oracle import core as oc
from oracle import philox as oph
from fuzz_states import place_fuzzed
from wide_cases import canon, oracle_state

B, CAP, STEPS = 37, 5, 9
SEED = 0x5EED0000BEEF
# (variant, agents, train): float4 rows (NA * (9R+1) % 4 == 0) and scalar rows, every kernel instance
VARIANTS = [("small", 4, False), ("medium", 8, False), ("medium", 1, False), ("medium", 3, False),
            ("medium", None, True), ("large", 16, False)]
IDS = ["small4", "medium8", "medium1", "medium3", "medium_train", "large16"]
GUARD = 256   # sentinel bytes after every output buffer


def place_near_end(env, lead=(3, 2, 1, 8)):
    """One step (so no env is fresh), then env e's clock to T - lead[e % 4]."""
    env.reset()
    env.vector_step(env.policy("greedy", 0.2), observe=False)
    c = canon(env)
    T = env.geometry["T"]
    c["t"] = (T - np.asarray(lead)[np.arange(env.B) % len(lead)]).astype(np.int32)
    env.from_canonical(c)


class Recording:
    """An env stepped through a ReplayBuffer's low-level methods, with what the oracle needs kept per
    recorded step: canonical and packed states before the step and after the un-reset step, actions,
    rewards, dones.  run(k) records up to step k."""

    def __init__(self, make, variant, na, train, capacity=CAP, place=None, actions=None):
        """`place(env)` puts the fresh env into its first state (default place_near_end); `actions(env,
        s)` gives step s's actions [B, NA] (default the greedy 0.3 policy of the env's state)."""
        import warehouse

        self.env = make(variant, B, na, train=train, seed=SEED)
        (place or place_near_end)(self.env)
        self.actions = actions or (lambda env, s: env.policy("greedy", 0.3).clone())
        self.buf = warehouse.ReplayBuffer(self.env, capacity)
        self.L = oc.layout_for(variant)
        self.T = self.env.geometry["T"]
        self.steps = []      # dicts per recorded step
        self.slot_step = {}  # slot -> recorded step it holds

    def run(self, upto):
        env, buf = self.env, self.buf
        while len(self.steps) < upto:
            s = len(self.steps)
            acts = self.actions(env, s)
            pre, pre_packed = canon(env), env.state.cpu().numpy().copy()
            slot = buf.cursor
            buf.put_obs(slot, acts)
            _, rew, done = env.vector_step(acts, autoreset=False, observe=False)
            post, post_packed = canon(env), env.state.cpu().numpy().copy()
            buf.put_next(slot)
            rec = dict(pre=pre, post=post, pre_packed=pre_packed, post_packed=post_packed,
                       actions=acts.cpu().numpy().copy(), rewards=rew.cpu().numpy().copy(),
                       dones=done.cpu().numpy().copy())
            rec["obs"] = ob.observe(self.L, oracle_state(pre)).astype(np.float32)
            rec["next_obs"] = ob.observe(self.L, oracle_state(post)).astype(np.float32)
            env.reset(mask=done)
            buf.advance()
            self.steps.append(rec)
            self.slot_step[slot] = s
        assert buf.filled == min(len(self.steps), buf.capacity) and buf.cursor == len(self.steps) % buf.capacity
        assert len(buf) == buf.filled * B
        return self

    def expected(self, idx):
        """What a gather of the (valid) indices idx must return, from the kept steps."""
        idx = np.asarray(idx, np.int64)
        slot, e = idx // B, idx % B
        st = np.array([self.slot_step[int(s)] for s in slot])
        pick = lambda key: np.stack([self.steps[k][key][j] for k, j in zip(st, e)])   # noqa: E731
        cols = lambda key: np.stack([self.steps[k][key][:, j] for k, j in zip(st, e)], axis=1)   # noqa: E731
        pre_n = np.array([self.steps[k]["pre"]["n"][j] for k, j in zip(st, e)])
        return dict(obs=pick("obs"), next_obs=pick("next_obs"), state=cols("pre_packed"),
                    next_state=cols("post_packed"), actions=pick("actions"), rewards=pick("rewards"),
                    dones=pick("dones"), n=np.minimum(pre_n, self.env.agent_slots).astype(np.int32), idx_out=idx,
                    step=st, env=e)


def guarded(buf, M, keys):
    """Caller-owned outputs for sample(out=...), each followed by GUARD sentinel bytes."""
    shapes = buf._shapes(M)
    raw, out = {}, {}
    for k in keys:
        shape, dt = shapes[k]
        nbytes = int(np.prod(shape)) * torch.empty((), dtype=dt).element_size()
        raw[k] = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=buf.env.device)
        out[k] = raw[k][:nbytes].view(dt).reshape(shape)
    return raw, out


def assert_guards(raw):
    for k, r in raw.items():
        assert bool((r[-GUARD:] == 0xA5).all()), f"bytes written past the end of {k}"


ALL_KEYS = ("obs", "next_obs", "state", "next_state", "actions", "rewards", "dones", "n", "idx_out")


def gather(buf, idx, keys=ALL_KEYS, draw=None):
    M = len(idx) if idx is not None else draw[0]
    raw, out = guarded(buf, M, keys)
    got = buf.sample(M, idx=idx, draw=None if draw is None else draw[1], out=out)
    assert_guards(raw)
    return {k: v.cpu().numpy() for k, v in got.items()}


def assert_batch(got, want, msg=""):
    for k in got:
        w = want[k]
        if k in ("state", "next_state"):
            w = w.view(np.int32) if w.dtype == np.uint32 else w
        np.testing.assert_array_equal(got[k], w, err_msg=f"{msg}{k}")


# ----------------------------------------------------------------------------- 1. round trip
def case_round_trip(make, variant, na, train):
    """Gathered obs / next_obs equal the oracle's rows of the captured states, state / next_state the
    packed states bit for bit (also through wh_unpack), the small outputs what was recorded; before the
    ring wraps (4 steps) and after (9 steps); a permutation of every entry, repeated entries, M = 1."""
    rec = Recording(make, variant, na, train)
    rng = np.random.default_rng(7)
    seen_done = seen_fresh = seen_dup = 0
    for upto in (4, STEPS):
        rec.run(upto)
        N = len(rec.buf)
        assert N == min(upto, CAP) * B
        dup = rng.integers(0, N, 185)
        dup[1::9] = dup[0]                                   # repeats, some adjacent in one workgroup
        for idx in (rng.permutation(N), dup, np.array([int(rng.integers(0, N))])):
            got, want = gather(rec.buf, idx), rec.expected(idx)
            assert_batch(got, {k: want[k] for k in got}, f"{variant}/{na} after {upto} steps, M={len(idx)}: ")
            seen_dup += len(np.unique(idx)) < len(idx)
            # a done sample's next_obs is the terminal observation (t = T), not a fresh one
            for m in np.flatnonzero(want["dones"]):
                post = rec.steps[want["step"][m]]["post"]
                assert post["t"][want["env"][m]] == rec.T and not post["fresh"][want["env"][m]]
                seen_done += 1
            # the step after a done one starts from the fresh post-reset state: all availabilities 0
            R = rec.L.R
            for m in range(len(idx)):
                if rec.steps[want["step"][m]]["pre"]["fresh"][want["env"][m]]:
                    live = got["obs"][m, : got["n"][m]]
                    assert live.shape[0] >= 1 and not live[:, 1:R].any() and not live[:, 9 * R - 4].any()
                    assert rec.steps[want["step"][m]]["pre"]["t"][want["env"][m]] == 0
                    seen_fresh += 1
        # the packed copies through wh_unpack: an env of M envs holding them is the captured state
        idx = rng.permutation(N)[:B]
        got, want = gather(rec.buf, idx, ("state", "next_state")), rec.expected(idx)
        for key, side in (("state", "pre"), ("next_state", "post")):
            twin = make(variant, B, na, train=train, seed=SEED)
            twin.state.copy_(torch.as_tensor(got[key]).to(twin.device))
            c = canon(twin)
            for f, v in c.items():
                ref = np.stack([rec.steps[k][side][f][j] for k, j in zip(want["step"], want["env"])])
                np.testing.assert_array_equal(v, ref, err_msg=f"{key}.{f}")
    assert len(rec.slot_step) == CAP and min(rec.slot_step.values()) == STEPS - CAP   # the ring wrapped
    assert seen_done >= 1 and seen_fresh >= 1 and seen_dup >= 1
    if train:
        assert len({int(n) for s in rec.steps for n in s["pre"]["n"]}) > 1   # variable agent counts


# ----------------------------------------------------------------------------- 1b. round trip, fuzzed
# place_fuzzed seeds per VARIANTS id, (full, sparse), chosen on the host engine so that the floors of
# case_round_trip_fuzzed hold at B = 37
FUZZ_SEEDS = {"small4": (101, 122), "medium8": (103, 104), "medium1": (105, 106), "medium3": (107, 108),
              "medium_train": (109, 110), "large16": (111, 112)}


def uniform_actions(seed):
    """actions(env, s) for Recording: seeded uniform integers in 0 .. 8 (no walk over the request
    table, so a sparse table is allowed)."""
    rng = np.random.default_rng(seed)

    def actions(env, s):
        a = rng.integers(0, 9, (env.B, env.agent_slots)).astype(np.int32)
        return torch.as_tensor(a).to(env.device)

    return actions


def fuzzed_recording(make, variant, na, train, full):
    seed = FUZZ_SEEDS[IDS[VARIANTS.index((variant, na, train))]][0 if full else 1]
    return Recording(make, variant, na, train, place=lambda env: place_fuzzed(env, full, seed),
                     actions=None if full else uniform_actions(seed))


def fuzz_coverage(rec):
    """What the recorded `pre` states of a Recording hold that place_near_end never reaches."""
    R = rec.L.R
    opened = [s["pre"]["pickup_target"] >= 0 for s in rec.steps]
    ring = sorted(rec.slot_step.values())
    return dict(
        expiring=sum(int((o & (s["pre"]["pickup_timer"] == 1)).sum()) for o, s in zip(opened, rec.steps)),
        expiring_below_w=sum(int((o & (s["pre"]["pickup_timer"] == 1) & (s["pre"]["t"] < rec.L.W - 1)[:, None]).sum())
                             for o, s in zip(opened, rec.steps)),
        steps_left=len(np.unique(np.concatenate([rec.steps[k]["pre"]["pickup_timer"][opened[k]] for k in ring]))),
        dones=sum(int(s["dones"].sum()) for s in rec.steps),
        rewards=sum(int((s["rewards"] != 0).sum()) for s in rec.steps),
        sparse=sum(int((o.sum(1) < R).sum()) for o in opened),
        after_done=sum(int(s["pre"]["episode"].astype(np.int64).clip(0, 1).sum()) for s in rec.steps))


def case_round_trip_fuzzed(make, variant, na, train, full):
    """case_round_trip's comparison from fuzz_states.place_fuzzed: after 4 and after 9 steps, a
    permutation of every entry and a batch with repeats equal the oracle's rows of the captured states,
    and the packed copies unpack to them.  full=False: sparse request tables and uniform actions.
    The coverage the parent's cases lack is asserted on the recorded pre-step states (floors well
    under what the host engine gives at B = 37): requests at timer 1 before a recorded step, distinct
    steps-left values in the final ring, dones, rewards, and with full=False states below R requests."""
    rec = fuzzed_recording(make, variant, na, train, full)
    rng = np.random.default_rng(13)
    for upto in (4, STEPS):
        rec.run(upto)
        N = len(rec.buf)
        assert N == min(upto, CAP) * B
        dup = rng.integers(0, N, 185)
        dup[1::9] = dup[0]
        for idx in (rng.permutation(N), dup):
            got, want = gather(rec.buf, idx), rec.expected(idx)
            assert set(got) == set(ALL_KEYS)
            assert_batch(got, {k: want[k] for k in got}, f"{variant}/{na} full={full} after {upto} steps, M={len(idx)}: ")
        idx = rng.permutation(N)[:B]
        got, want = gather(rec.buf, idx, ("state", "next_state")), rec.expected(idx)
        for key, side in (("state", "pre"), ("next_state", "post")):
            twin = make(variant, B, na, train=train, seed=SEED)
            twin.state.copy_(torch.as_tensor(got[key]).to(twin.device))
            c = canon(twin)
            for f, v in c.items():
                ref = np.stack([rec.steps[k][side][f][j] for k, j in zip(want["step"], want["env"])])
                np.testing.assert_array_equal(v, ref, err_msg=f"{key}.{f}")
    assert len(rec.slot_step) == CAP and min(rec.slot_step.values()) == STEPS - CAP   # the ring wrapped
    cov = fuzz_coverage(rec)
    print(f"coverage {variant}/{na} train={train} full={full}: {cov}")
    assert cov["expiring"] >= 20 and cov["expiring_below_w"] >= 1, cov
    assert cov["steps_left"] >= 60, cov
    assert cov["dones"] >= 10 and cov["rewards"] >= 1 and cov["after_done"] >= 1, cov
    if full:
        assert cov["sparse"] == 0, cov
    else:
        assert cov["sparse"] >= 1, cov
    return cov


# ----------------------------------------------------------------------------- 2. trajectory
def case_step_keeps_trajectory(make, variant, na, train):
    """ReplayBuffer.step is vector_step(autoreset=True): two envs with one seed, one stepped through
    the buffer; states, rewards, dones, rows and episode-stat bins equal at each of 12 steps."""
    import warehouse

    envs = [make(variant, B, na, train=train, seed=SEED) for _ in range(2)]
    for e in envs:
        place_near_end(e, lead=(6, 5, 4, 9))
        e.enable_episode_stats()
    buf = warehouse.ReplayBuffer(envs[0], CAP)
    finished, n_seen = 0, set()
    for s in range(12):
        acts = envs[1].policy("greedy", 0.3).clone()
        a = buf.step(acts)
        b = envs[1].vector_step(acts, autoreset=True)
        for x, y, what in zip(a, b, ("obs", "rewards", "dones")):
            assert torch.equal(x.cpu(), y.cpu()), f"{what} differ at step {s}"
        assert torch.equal(envs[0].state.cpu(), envs[1].state.cpu()), f"state differs at step {s}"
        ba, bb = envs[0].stats.bins(), envs[1].stats.bins()
        for k in ba:
            np.testing.assert_array_equal(ba[k], bb[k], err_msg=f"stats {k} at step {s}")
        assert torch.equal(envs[0].stats.episode_return.cpu(), envs[1].stats.episode_return.cpu())
        finished += int(b[2].sum())
        n_seen |= {int(n) for n in canon(envs[1])["n"]}
        assert buf.cursor == (s + 1) % CAP and buf.filled == min(s + 1, CAP)
    assert finished >= B and int(envs[1].stats.bins()["episodes"].sum()) == finished   # every env crossed an episode end
    if train:
        assert len(n_seen) > 1


# ----------------------------------------------------------------------------- 3. device index draw
def expected_draw(seed, draw, M, filled):
    m = np.arange(M, dtype=np.uint64)
    c = oph.philox4x32_10(m, draw & 0xFFFFFFFF, draw >> 32, 6 << 24, seed & 0xFFFFFFFF, seed >> 32)
    return oph.uniform_int(filled, c[0]) * B + oph.uniform_int(B, c[1])


def case_index_draw(make):
    """idx=None: idx_out is the philox contract's (purpose 6) for filled = 1, 3, 5; the same (seed,
    draw) gives the same batch, another draw another one, and the batch is the explicit gather of
    idx_out."""
    rec = Recording(make, "medium", 8, False)
    M = 70
    for upto, filled in ((1, 1), (3, 3), (STEPS, CAP)):
        rec.run(upto)
        assert rec.buf.filled == filled
        draw = (3 << 32) | (5 + upto)
        a = gather(rec.buf, None, draw=(M, draw))
        want = expected_draw(SEED, draw, M, filled)
        np.testing.assert_array_equal(a["idx_out"], want)
        assert a["idx_out"].min() >= 0 and a["idx_out"].max() < filled * B
        assert len(np.unique(a["idx_out"] // B)) == filled              # every filled slot drawn from
        assert_batch(gather(rec.buf, None, draw=(M, draw)), a, "same draw: ")
        other = gather(rec.buf, None, draw=(M, draw + (1 << 32)))
        assert not np.array_equal(other["idx_out"], a["idx_out"])
        np.testing.assert_array_equal(other["idx_out"], expected_draw(SEED, draw + (1 << 32), M, filled))
        assert_batch(gather(rec.buf, a["idx_out"]), a, "explicit idx_out: ")
        assert_batch(a, {k: rec.expected(want)[k] for k in a}, "oracle: ")
    # the buffer's own counter: consecutive default draws are draws 0, 1
    rec.buf._draw = 0
    for d in (0, 1):
        np.testing.assert_array_equal(rec.buf.sample(M)["idx_out"].cpu().numpy(), expected_draw(SEED, d, M, CAP))


# ----------------------------------------------------------------------------- 4. invalid indices
def case_invalid_indices(make, variant, na, train):
    """An index outside [0, filled * B) gives n = -1 and zeroes every other output of its sample;
    valid neighbours are unaffected and nothing is written past any buffer."""
    rec = Recording(make, variant, na, train).run(3)
    N = len(rec.buf)
    assert N == 3 * B
    rng = np.random.default_rng(3)
    idx = rng.integers(0, N, 90)
    bad_at = np.array([0, 1, 17, 63, 64, 65, 89])
    idx[bad_at] = [-1, N, 1 << 62, -(1 << 62), N + B, CAP * B, N]   # (slots 3, 4 exist but are not filled)
    good = np.setdiff1d(np.arange(len(idx)), bad_at)
    got = gather(rec.buf, idx)
    want = rec.expected(idx[good])
    for k, v in got.items():
        axis = 1 if k in ("state", "next_state") else 0
        np.testing.assert_array_equal(np.take(v, good, axis=axis), want[k].view(v.dtype) if axis else want[k],
                                      err_msg=k)
        bad = np.take(v, bad_at, axis=axis)
        if k == "n":
            assert (bad == -1).all()
        else:
            assert not bad.any(), f"{k} of an invalid sample is not zero"
    assert (got["n"][good] >= 1).all()


# ----------------------------------------------------------------------------- 5. fragments (device)
def case_fragments(make, variant, na, rec=None, rows=False):
    """xfrag / next_xfrag are byte-equal to wh_observe_x on the gathered state / next_state planes as
    a batch of M envs: M with whole 32-row tiles, and M with a tail tile.  `rec`: a finished Recording
    to gather from (default: one from place_near_end).  `rows`: also the gathered obs / next_obs
    against wh_observe on the same planes."""
    rec = rec or Recording(make, variant, na, False).run(STEPS)
    N = len(rec.buf)
    rng = np.random.default_rng(5)
    for M in (64, 37, 1):
        idx = rng.integers(0, N, M)
        idx[M // 2] = -1                                       # an invalid sample among them
        keys = ("xfrag", "next_xfrag", "state", "next_state", "n") + (("obs", "next_obs") if rows else ())
        raw, out = guarded(rec.buf, M, keys)
        got = rec.buf.sample(M, idx=idx, out=out)
        assert_guards(raw)
        assert got["n"][M // 2].item() == -1
        assert (M * na) % 32 == 0 or M != 64
        twin = make(variant, M, na, seed=SEED)
        for fk, sk, ok in (("xfrag", "state", "obs"), ("next_xfrag", "next_state", "next_obs")):
            twin.state.copy_(got[sk])
            ref = twin.observe_x()
            assert ref.shape == got[fk].shape
            assert torch.equal(ref, got[fk]), f"{fk} differs (M = {M})"
            if rows:
                assert torch.equal(twin.observe(), got[ok]), f"{ok} differs from wh_observe of {sk} (M = {M})"


def case_fragments_fuzzed(make, variant, na):
    """case_fragments on a fuzzed recording (small steps-left values, crowded agents, clocks from 0 to
    T; full and sparse request tables), with the gathered rows against wh_observe of the gathered planes."""
    for full in (True, False):
        case_fragments(make, variant, na, rec=fuzzed_recording(make, variant, na, False, full).run(STEPS), rows=True)


# ----------------------------------------------------------------------------- 6. portability (device)
def case_ring_portability(make, make_host, variant, na, train):
    """A ring recorded on the device and copied to host memory gives, gathered by the host engine,
    the batch the device gather gives."""
    import warehouse

    rec = Recording(make, variant, na, train).run(STEPS)
    host = warehouse.ReplayBuffer(make_host(variant, B, na, train=train, seed=SEED), CAP)
    for name in ("states", "actions", "rewards", "dones"):
        getattr(host, name).copy_(getattr(rec.buf, name).cpu())
    host._filled, host._cursor = rec.buf.filled, rec.buf.cursor
    idx = np.random.default_rng(9).integers(-2, len(rec.buf) + 2, 101)
    assert_batch(gather(host, idx), gather(rec.buf, idx), "host vs device: ")
    draw = (1 << 40) | 3
    assert_batch(gather(host, None, draw=(50, draw)), gather(rec.buf, None, draw=(50, draw)), "drawn: ")


# ----------------------------------------------------------------------------- 7. refusals
def case_refusals(nat, lib, host: bool):
    """The host-checkable refusals of wh_replay_put / wh_replay_gather: codes of one library, as a
    list (the caller compares the two libraries' lists).  Pointers are dummies that a refused call
    never dereferences, except on the host engine, where they are real sentinel-filled buffers that
    must stay untouched."""
    cfg = nat.make_config(12, 4, (4, 8), 4, 200, 200)          # small/4: words 14, rows 148 floats (float4)
    Bc, cap, M, words, na, L = 3, 2, 5, 14, 4, 37
    keep = []

    def mem(nbytes):
        if not host:
            return 4096 * (len(keep) + 1)                       # never dereferenced: refused first
        t = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8)
        keep.append(t)
        return t.data_ptr()

    ring = dict(states=mem(cap * 2 * Bc * words * 4), actions=mem(cap * Bc * na), rewards=mem(cap * Bc * na * 4),
                dones=mem(cap * Bc), capacity=cap)
    state, acts, rew, done = mem(words * Bc * 4), mem(Bc * na * 4), mem(Bc * na * 4), mem(Bc)
    outs = dict(obs=mem(M * na * L * 4), next_obs=mem(M * na * L * 4), xfrag=None, next_xfrag=None,
                state=mem(words * M * 4), next_state=mem(words * M * 4), actions=mem(M * na * 4),
                rewards=mem(M * na * 4), dones=mem(M), n=mem(M * 4), idx_out=mem(M * 8))
    idx = mem(M * 8)

    def put(B=Bc, ring_=ring, slot=0, stage=0, state_=state, a=acts, r=rew, d=done, cfg_=cfg):
        rp = None if ring_ is None else ctypes.byref(nat.WhReplayRing(**ring_))
        return lib.wh_replay_put(ctypes.byref(cfg_), B, rp, slot, stage, state_, a, r, d, None)

    def gat(B=Bc, ring_=ring, filled=1, M_=M, idx_=idx, outs_=outs, cfg_=cfg):
        rp = None if ring_ is None else ctypes.byref(nat.WhReplayRing(**ring_))
        bp = None if outs_ is None else ctypes.byref(nat.WhReplayBatch(**outs_))
        return lib.wh_replay_gather(ctypes.byref(cfg_), B, rp, filled, M_, idx_, 1, 2, bp, None)

    E, OK = nat.WH_EINVAL, nat.WH_OK
    bad_cfg = nat.make_config(12, 4, (4, 8), 0, 200, 200)
    border = nat.make_config(12, 4, (1, 8), 4, 200, 200)
    none = {k: None for k in outs}
    table = [
        ("put: NULL ring", put(ring_=None), E),
        ("put: capacity 0", put(ring_=dict(ring, capacity=0)), E),
        ("put: slot -1", put(slot=-1), E),
        ("put: slot = capacity", put(slot=cap), E),
        ("put: stage 2", put(stage=2), E),
        ("put: stage -1", put(stage=-1), E),
        ("put: NULL ring states", put(ring_=dict(ring, states=None)), E),
        ("put 0: NULL ring actions", put(ring_=dict(ring, actions=None)), E),
        ("put 0: NULL actions", put(a=None), E),
        ("put 1: NULL ring rewards", put(stage=1, ring_=dict(ring, rewards=None)), E),
        ("put 1: NULL ring dones", put(stage=1, ring_=dict(ring, dones=None)), E),
        ("put 1: NULL rewards", put(stage=1, r=None), E),
        ("put 1: NULL dones", put(stage=1, d=None), E),
        ("put: NULL state", put(state_=None), E),
        ("put: B < 0", put(B=-1), E),
        ("put: bad config", put(cfg_=bad_cfg), E),
        ("put: racks on the border", put(cfg_=border), nat.WH_ENOTSUP),
        ("put: bad option before bad config", put(stage=2, cfg_=border), E),
        ("put: B = 0", put(B=0, state_=None, a=None), OK),
        ("gather: NULL ring", gat(ring_=None), E),
        ("gather: capacity 0", gat(ring_=dict(ring, capacity=0)), E),
        ("gather: filled 0", gat(filled=0), E),
        ("gather: filled > capacity", gat(filled=cap + 1), E),
        ("gather: M < 0", gat(M_=-1), E),
        ("gather: NULL batch", gat(outs_=None), E),
        ("gather: all outputs NULL", gat(outs_=none), E),
        ("gather: all outputs NULL, M = 0", gat(outs_=none, M_=0), E),
        ("gather: NULL ring states", gat(ring_=dict(ring, states=None)), E),
        ("gather: actions without ring actions", gat(ring_=dict(ring, actions=None)), E),
        ("gather: rewards without ring rewards", gat(ring_=dict(ring, rewards=None)), E),
        ("gather: dones without ring dones", gat(ring_=dict(ring, dones=None)), E),
        ("gather: obs not 16-byte aligned", gat(outs_=dict(outs, obs=outs["obs"] + 4)), E),
        ("gather: next_obs not 16-byte aligned", gat(outs_=dict(outs, next_obs=outs["next_obs"] + 8)), E),
        ("gather: xfrag not 16-byte aligned", gat(outs_=dict(outs, xfrag=outs["state"] + 4)), E),
        ("gather: next_xfrag not 16-byte aligned", gat(outs_=dict(outs, next_xfrag=outs["state"] + 8)), E),
        ("gather: B < 0", gat(B=-1), E),
        ("gather: bad config", gat(cfg_=bad_cfg), E),
        ("gather: racks on the border", gat(cfg_=border), nat.WH_ENOTSUP),
        ("gather: M = 0", gat(M_=0), OK),
        ("gather: B = 0", gat(B=0), OK),
        ("gather: M = 0, no ring buffers", gat(M_=0, ring_=dict(ring, states=None, actions=None)), OK),
    ]
    for what, rc, want in table:
        assert rc == want, f"{what}: got {rc}, expected {want}"
    for t in keep:
        assert bool((t == 0xA5).all()), "a refused (or empty) call wrote to a buffer"
    return [(what, rc) for what, rc, _ in table]
