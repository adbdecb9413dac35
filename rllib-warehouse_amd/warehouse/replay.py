"""Off-policy replay for a `BatchedWarehouse`: a ring of packed transitions on the env's device and
a gather that turns a sampled minibatch of ring entries straight into learner inputs
(include/warehouse_amd.h, REPLAY RING; csrc/replay.h).

A transition is stored as two packed states (before the step; after it and before any reset) plus
its actions, rewards and done flag -- 265 bytes per Medium-8 env-step against 5,289 as f32 rows --
because every observation row is a function of the packed state.  `sample()` images the sampled
records into `obs` / `next_obs` rows, the policy network's fragment operand, and/or plane-major
packed states, in one launch.

    buf = ReplayBuffer(env, capacity=200)
    obs, rew, done = buf.step(actions)           # a recorded vector_step(autoreset=True)
    obs, rew, done = buf.collect(100, "greedy", 0.1)   # 100 recorded sampler steps, one launch
    batch = buf.sample(64)                       # obs, next_obs, actions, rewards, dones, n, idx_out

With `prioritized=True` the buffer also keeps a priority tree over its entries (include/
warehouse_amd.h, REPLAY PRIORITIES; csrc/prio.h): a recorded slot enters at the largest priority seen
so far, `sample()` draws entries in proportion to their priority and returns importance weights,
and `update_priorities()` writes the learner's new ones.  All of it is integer arithmetic on the
device (or the host engine), exact and the same on both, with no host sync.

    buf = ReplayBuffer(env, capacity=200, prioritized=True)
    batch = buf.sample(64, beta=0.4)             # ... plus prio_q, weights
    buf.update_priorities(batch["idx_out"], td_error)

`dones` is what the step reported; a learner that follows the reference's `no_done_at_end: true`
ignores it at the bootstrap, and `next_obs` of such a sample is the terminal observation (not the
first one of the next episode).
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import numpy as np
import torch

from . import _native as nat
from .batched import POLICIES, BatchedWarehouse, _check_out, _dev_i32

# fused=None takes the one record launch (wh_replay_record) on every lane-per-env env: at each measured
# shape its median is below the five launches' minimum over the rounds (DESIGN.md §5.12,
# profiles/replay_record_probe.txt; one MI355X, us per recorded step with f32 rows, record launch /
# five launches): Medium-8 B = 65,536 45.1 / 60.0, B = 4,096 17.6 / 26.9, B = 256 16.0 / 26.0,
# Large-16 B = 65,536 120.2 / 140.6; with the fragment operand 39.4 / 52.6, 19.7 / 29.3, 18.5 / 26.4,
# 91.8 / 117.0.  So there is no batch-size threshold to keep.

_SIDES = (("obs", "next_obs"), ("xfrag", "next_xfrag"), ("state", "next_state"))


class ReplayBuffer:
    """A ring of `capacity` time steps of every env of `env` (slot = one step of all B envs), on
    the env's device with the env's engine (device="cpu": the host engine, no fragments)."""

    def __init__(self, env: BatchedWarehouse, capacity: int, prioritized: bool = False, alpha: float = 0.6,
                 eps: float = 1e-6, fused: Optional[bool] = None):
        """`prioritized`: keep a priority tree (RLlib's `prioritized_replay`), with RLlib's
        `prioritized_replay_alpha` and `prioritized_replay_eps` as `alpha` and `eps`.
        `fused`: True records a step() / collect() inside the step launch (wh_replay_record: one
        launch, plus the rows), False with the five launches put, step, put, reset, observe; None
        (default) takes the one launch too (it measured faster at every shape).  An env with
        lanes_per_env=16 always takes the five launches.  Both routes write the same bytes;
        `last_fused` says which one the last step() or collect() took."""
        capacity = int(capacity)
        if capacity < 1:
            raise ValueError(f"capacity: at least 1 slot, got {capacity}")
        self.env = env
        self.capacity = capacity
        B, NA, W, d = env.B, env.agent_slots, env.layout.words_per_env, env.device
        self.states = torch.zeros((capacity, 2, B, W), dtype=torch.int32, device=d)
        self.actions = torch.zeros((capacity, B, NA), dtype=torch.uint8, device=d)
        self.rewards = torch.zeros((capacity, B, NA), dtype=torch.float32, device=d)
        self.dones = torch.zeros((capacity, B), dtype=torch.uint8, device=d)
        self._ring = nat.WhReplayRing(self.states.data_ptr(), self.actions.data_ptr(), self.rewards.data_ptr(),
                                      self.dones.data_ptr(), capacity)
        self._cursor = 0
        self._filled = 0
        self._draw = 0
        self._out: Dict[tuple, torch.Tensor] = {}
        self.fused = None if fused is None else bool(fused)
        self.last_fused: Optional[bool] = None
        self.prioritized = bool(prioritized)
        if self.prioritized:
            self._init_tree(float(alpha), float(eps))

    def _init_tree(self, alpha: float, eps: float) -> None:
        """The empty tree: all-zero leaves and sums, max_q = priority 1.0.  Leaves and max_q are
        int32 and the sums int64 tensors: a stored q is below 2^31 and a sum below 2^62, so the
        signed views hold the same numbers."""
        e = self.env
        count = self.capacity * e.B
        if not (alpha >= 0.0 and eps >= 0.0):
            raise ValueError(f"alpha and eps: not negative, got {alpha}, {eps}")
        lw, nw, lv = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
        nat.check(e._lib.wh_replay_prio_query(count, ctypes.byref(lw), ctypes.byref(nw), ctypes.byref(lv)),
                  "wh_replay_prio_query")
        self.alpha, self.eps = alpha, eps
        self.prio_levels = lv.value
        self.prio_leaf = torch.zeros(lw.value, dtype=torch.int32, device=e.device)
        self.prio_node = torch.zeros(nw.value, dtype=torch.int64, device=e.device)
        self.prio_max_q = torch.full((1,), nat.WH_PRIO_ONE, dtype=torch.int32, device=e.device)
        self.prio_total = torch.zeros(1, dtype=torch.int64, device=e.device)
        self._tree = nat.WhReplayPrio(self.prio_leaf.data_ptr(), self.prio_node.data_ptr(),
                                      self.prio_max_q.data_ptr(), count)

    def _prio_call(self, name, *args) -> None:
        nat.check(getattr(self.env._lib, name)(ctypes.byref(self._tree), *args), name)

    # ------------------------------------------------------------------ recording
    @property
    def cursor(self) -> int:
        """The slot the next step() records into."""
        return self._cursor

    @property
    def filled(self) -> int:
        """Slots that hold a whole transition (what sample() draws from)."""
        return self._filled

    def __len__(self) -> int:
        return self._filled * self.env.B

    def _put(self, slot: int, stage: int, actions=None) -> None:
        e = self.env
        slot = int(slot)
        if not 0 <= slot < self.capacity:
            raise ValueError(f"slot: 0 .. {self.capacity - 1}, got {slot}")
        e._call("wh_replay_put", ctypes.byref(self._ring), slot, stage, e.state.data_ptr(),
                None if actions is None else actions.data_ptr(),
                e.rewards.data_ptr() if stage else None, e.dones.data_ptr() if stage else None, e.stream)

    def put_obs(self, slot: int, actions=None) -> None:
        """Record the env's current state as the state `actions` ([B, NA], 0..8; None = env.actions,
        what env.policy() wrote) were chosen from (side 0 of `slot`), with the actions."""
        e = self.env
        self._put(slot, 0, _dev_i32(e.actions if actions is None else actions, e.device, (e.B, e.agent_slots)))

    def put_next(self, slot: int) -> None:
        """Record the env's current state as the outcome (side 1 of `slot`) with the env's reward and
        done buffers: call it after a step WITHOUT auto-reset and before resetting the done envs."""
        self._put(slot, 1)

    def advance(self) -> None:
        """Count the slot at the cursor as filled and move on (step() does this itself).  A
        prioritized buffer gives the slot's entries the largest priority seen so far."""
        if self.prioritized:
            self._prio_call("wh_replay_prio_fill", self._cursor * self.env.B, self.env.B, 1, 0, self.env.stream)
        self._cursor = (self._cursor + 1) % self.capacity
        self._filled = min(self._filled + 1, self.capacity)

    def _record_route(self) -> bool:
        """Does the next recorded step take the one record launch (wh_replay_record)?  The wide
        (16 lanes per env) form has no record kernel; `fused=None` takes it wherever there is one."""
        return self.env.lanes_per_env == 1 and self.fused is not False

    def _rows(self, observe: bool, frag: bool):
        """The output of the step's rows: (obs tensor or None, fragment buffer or None)."""
        e = self.env
        if not observe:
            return None, None
        if frag:
            return None, e._xfrag_buffer()
        if e._obs is None:
            e._obs = torch.empty((e.B, e.agent_slots, e.obs_len), dtype=torch.float32, device=e.device)
        return e._obs, None

    def _record(self, steps: int, policy: int, p: float, actions, rewards, dones, obs, xf) -> None:
        e = self.env
        e._call("wh_replay_record", e.state.data_ptr(), ctypes.byref(self._ring), self._cursor, steps, policy, p,
                None if actions is None else actions.data_ptr(), rewards.data_ptr(), dones.data_ptr(),
                None if obs is None else obs.data_ptr(), None if xf is None else xf.data_ptr(),
                None if e.stats is None else e.stats.ref, int(e.train), e.seed, e.env_offset, e.stream)

    def _unfused_step(self, a) -> None:
        """One recorded step as five launches: put, step without auto-reset, put, reset of the done envs."""
        e = self.env
        self._put(self._cursor, 0, a)
        e.vector_step(a, autoreset=False, observe=False)
        self._put(self._cursor, 1)
        e.reset(mask=e.dones)

    @staticmethod
    def _operand(operand: str, host: bool) -> bool:
        if operand not in ("rows", "fragments"):
            raise ValueError("operand must be 'rows' or 'fragments'")
        if operand == "fragments" and host:
            raise nat.WarehouseNativeError("the fragment operand is a device format (the host engine has none)")
        return operand == "fragments"

    def step(self, actions, observe: bool = True, operand: str = "rows"):
        """env.vector_step(actions, autoreset=True), recorded: the same trajectory (philox draws,
        Train-variant n redraws, episode stats) and the same return value.  operand="fragments"
        (device only) returns the env's observe_x() buffer -- the policy network's layer-0 operand,
        what vector_step_x returns -- instead of the f32 rows.  On a lane-per-env env the step is
        one record launch (wh_replay_record) plus the rows (see `fused`); `last_fused` says which
        route ran."""
        e = self.env
        frag = self._operand(operand, e.host)
        a = _dev_i32(actions, e.device, (e.B, e.agent_slots))
        self.last_fused = self._record_route()
        if self.last_fused:
            obs, xf = self._rows(observe, frag)
            self._record(1, nat.WH_POLICY_EXTERNAL, 0.0, a, e.rewards, e.dones, obs, xf)
        else:
            self._unfused_step(a)
            obs, xf = None, None
            if observe:
                obs, xf = (None, e.observe_x()) if frag else (e.observe(), None)
        self.advance()
        return (xf if frag else obs), e.rewards, e.dones

    def collect(self, steps: int, policy: str = "greedy", p: float = 0.0, observe: bool = True,
                operand: str = "rows"):
        """`steps` (<= capacity) recorded sampler steps with the device policy -- env.policy(policy, p)
        then step(), `steps` times -- in one launch on a lane-per-env env, so a buffer fills without
        a Python loop.  Returns (the final state's obs or fragment buffer, or None; rewards
        [steps,B,NA]; dones [steps,B]), the two outputs fresh tensors."""
        e = self.env
        steps = int(steps)
        if not 0 <= steps <= self.capacity:
            raise ValueError(f"steps: 0 .. capacity ({self.capacity}), got {steps}")
        frag = self._operand(operand, e.host)
        pol = POLICIES[policy]
        rew = torch.empty((steps, e.B, e.agent_slots), dtype=torch.float32, device=e.device)
        done = torch.empty((steps, e.B), dtype=torch.uint8, device=e.device)
        self.last_fused = self._record_route() and steps > 0
        if self.last_fused:
            obs, xf = self._rows(observe, frag)
            self._record(steps, pol, float(p), None, rew, done, obs, xf)
            if self.prioritized:   # the new slots enter at the largest priority: the range, or its two parts
                first = min(steps, self.capacity - self._cursor)
                for slot, count in ((self._cursor, first), (0, steps - first)):
                    if count:
                        self._prio_call("wh_replay_prio_fill", slot * e.B, count * e.B, 1, 0, e.stream)
            self._cursor = (self._cursor + steps) % self.capacity
            self._filled = min(self._filled + steps, self.capacity)
        else:
            for k in range(steps):
                self._unfused_step(e.policy(policy, p))
                rew[k].copy_(e.rewards)
                done[k].copy_(e.dones)
                self.advance()
            obs, xf = None, None
            if observe:
                obs, xf = (None, e.observe_x()) if frag else (e.observe(), None)
        return (xf if frag else obs), rew, done

    def update_priorities(self, idx, priorities) -> None:
        """Entry idx[m] (slot * B + env, what sample() returned as idx_out) gets the priority
        (|priorities[m]| + eps) ** alpha, computed in f32 and quantised by the tree's rule.  An index
        outside the ring is ignored; of duplicate indices the largest priority wins."""
        if not self.prioritized:
            raise ValueError("update_priorities: the buffer was made with prioritized=False")
        e = self.env
        ix = torch.as_tensor(np.asarray(idx) if not torch.is_tensor(idx) else idx)
        ix = ix.to(device=e.device, dtype=torch.int64).contiguous()
        pr = torch.as_tensor(np.asarray(priorities) if not torch.is_tensor(priorities) else priorities)
        pr = pr.to(device=e.device, dtype=torch.float32)
        if ix.dim() != 1 or pr.shape != ix.shape:
            raise ValueError(f"idx and priorities: two [M] vectors, got {tuple(ix.shape)} and {tuple(pr.shape)}")
        p = ((pr.abs() + self.eps) ** self.alpha).contiguous()
        if ix.numel():
            self._prio_call("wh_replay_prio_update", ix.numel(), ix.data_ptr(), p.data_ptr(), e.stream)

    # ------------------------------------------------------------------ sampling
    def _shapes(self, M: int):
        e = self.env
        NA, L, W = e.agent_slots, e.obs_len, e.layout.words_per_env
        frag = ((M * NA + 31) // 32, (L + 2 + 15) // 16, 64, 16)
        return dict(obs=((M, NA, L), torch.float32), next_obs=((M, NA, L), torch.float32),
                    xfrag=(frag, torch.uint8), next_xfrag=(frag, torch.uint8),
                    state=((W, M), torch.int32), next_state=((W, M), torch.int32),
                    actions=((M, NA), torch.int32), rewards=((M, NA), torch.float32), dones=((M,), torch.uint8),
                    n=((M,), torch.int32), idx_out=((M,), torch.int64))

    def _own(self, k: str, M: int, shape, dt) -> torch.Tensor:
        if (k, M) not in self._out:
            self._out = {kk: v for kk, v in self._out.items() if kk[0] != k}   # one size kept per key
            self._out[(k, M)] = torch.empty(shape, dtype=dt, device=self.env.device)
        return self._out[(k, M)]

    def sample(self, M: int, idx=None, draw: Optional[int] = None, *, rows: bool = True, fragments: bool = False,
               states: bool = False, out: Optional[Dict[str, torch.Tensor]] = None, beta: float = 0.4,
               uniform: bool = False) -> Dict[str, torch.Tensor]:
        """M transitions as a dict of tensors: actions [M,NA] int32, rewards [M,NA], dones [M] uint8,
        n [M] (live agents; -1 = invalid index), idx_out [M] int64, and per request obs / next_obs
        [M,NA,9R+1] (rows), xfrag / next_xfrag (fragments: the policy network's operand for a batch
        of M envs), state / next_state [words, M] (states).  `idx` [M] (slot * B + env; duplicates
        allowed, an index outside [0, len(self)) gives an all-zero sample with n = -1) lets a
        prioritized sampler supply its own indices; None draws them on the device from
        (env.seed, draw), `draw` defaulting to a counter the buffer keeps.  The tensors are the
        buffer's own, overwritten by the next call -- or the caller's, through `out` (exactly the
        keys to write).

        A prioritized buffer with idx=None (and not `uniform`) draws entry i with probability
        q_i / total from its tree instead (philox purpose 7 on (env.seed, draw)) and gathers those
        entries on the same stream, with no host sync.  The dict then also holds prio_q [M] int32,
        the sampled entries' fixed-point priorities, and weights [M] f32 = (q / total * N) ** -beta
        divided by the batch's largest weight, N = len(self), computed in float64 from the exact
        integers (`beta`: RLlib's prioritized_replay_beta); `self.prio_total` [1] int64 is the
        total that launch read.  RLlib normalises by the weight of the
        smallest priority in the whole buffer rather than in the batch; the two differ by one
        common factor per batch, which rescales that batch's loss and nothing else.  `idx=...` and
        `uniform=True` are the plain paths above, whatever the buffer."""
        e = self.env
        M = int(M)
        if M < 0:
            raise ValueError(f"M: a sample count, got {M}")
        if self._filled < 1:
            raise ValueError("sample: the buffer holds no transition yet")
        if fragments and e.host:
            raise nat.WarehouseNativeError("sample: the fragment operand is a device format (the host engine has none)")
        shapes = self._shapes(M)
        if out is None:
            keys = ["actions", "rewards", "dones", "n", "idx_out"]
            for on, pair in zip((rows, fragments, states), _SIDES):
                if on:
                    keys += pair
            t = {}
            for k in keys:
                t[k] = self._own(k, M, *shapes[k])
        else:
            t = dict(out)
            for k, v in t.items():
                if k not in shapes:
                    raise ValueError(f"out: unknown key {k!r}")
                _check_out(v, *shapes[k], e.device)
            if not t:
                raise ValueError("out: no output tensor")
        ix = None
        if idx is not None:
            ix = torch.as_tensor(np.asarray(idx) if not torch.is_tensor(idx) else idx)
            if tuple(ix.shape) != (M,):
                raise ValueError(f"idx: expected shape ({M},), got {tuple(ix.shape)}")
            ix = ix.to(device=e.device, dtype=torch.int64).contiguous()
        elif draw is None:
            draw = self._draw
            self._draw += 1
        draw = int(draw or 0) & 0xFFFFFFFFFFFFFFFF
        by_priority = self.prioritized and idx is None and not uniform
        if by_priority:
            t["prio_q"] = self._own("prio_q", M, (M,), torch.int32)
            if M:
                ix = self._own("prio_idx", M, (M,), torch.int64)
                self._prio_call("wh_replay_prio_sample", M, None, e.seed, draw, ix.data_ptr(),
                                t["prio_q"].data_ptr(), self.prio_total.data_ptr(), e.stream)
            # (q / total * N) ** -beta over the batch's largest such weight: N / total is common to
            # both and cancels, leaving (q / the batch's smallest q) ** -beta -- half the small
            # launches.  (An empty tree gives q = 0 throughout: weights 1 for its n = -1 samples.)
            q = t["prio_q"].clamp(min=1).to(torch.float64)
            t["weights"] = ((q / q.min()) ** -float(beta) if M else q).to(torch.float32)
        if M == 0:
            return t
        p = {k: (t[k].data_ptr() if k in t else None) for k in shapes}
        batch = nat.WhReplayBatch(p["obs"], p["next_obs"], p["xfrag"], p["next_xfrag"], p["state"], p["next_state"],
                                  p["actions"], p["rewards"], p["dones"], p["n"], p["idx_out"])
        e._call("wh_replay_gather", ctypes.byref(self._ring), self._filled, M, e._ptr(ix), e.seed, draw,
                ctypes.byref(batch), e.stream)
        return t
