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
    batch = buf.sample(64)                       # obs, next_obs, actions, rewards, dones, n, idx_out

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
from .batched import BatchedWarehouse, _check_out, _dev_i32

_SIDES = (("obs", "next_obs"), ("xfrag", "next_xfrag"), ("state", "next_state"))


class ReplayBuffer:
    """A ring of `capacity` time steps of every env of `env` (slot = one step of all B envs), on
    the env's device with the env's engine (device="cpu": the host engine, no fragments)."""

    def __init__(self, env: BatchedWarehouse, capacity: int):
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
        """Count the slot at the cursor as filled and move on (step() does this itself)."""
        self._cursor = (self._cursor + 1) % self.capacity
        self._filled = min(self._filled + 1, self.capacity)

    def step(self, actions, observe: bool = True):
        """env.vector_step(actions, autoreset=True), recorded: the same trajectory (philox draws,
        Train-variant n redraws, episode stats) and the same return value."""
        e = self.env
        a = _dev_i32(actions, e.device, (e.B, e.agent_slots))
        self._put(self._cursor, 0, a)
        e.vector_step(a, autoreset=False, observe=False)
        self._put(self._cursor, 1)
        e.reset(mask=e.dones)
        obs = e.observe() if observe else None
        self.advance()
        return obs, e.rewards, e.dones

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

    def sample(self, M: int, idx=None, draw: Optional[int] = None, *, rows: bool = True, fragments: bool = False,
               states: bool = False, out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """M transitions as a dict of tensors: actions [M,NA] int32, rewards [M,NA], dones [M] uint8,
        n [M] (live agents; -1 = invalid index), idx_out [M] int64, and per request obs / next_obs
        [M,NA,9R+1] (rows), xfrag / next_xfrag (fragments: the policy network's operand for a batch
        of M envs), state / next_state [words, M] (states).  `idx` [M] (slot * B + env; duplicates
        allowed, an index outside [0, len(self)) gives an all-zero sample with n = -1) lets a
        prioritized sampler supply its own indices; None draws them on the device from
        (env.seed, draw), `draw` defaulting to a counter the buffer keeps.  The tensors are the
        buffer's own, overwritten by the next call -- or the caller's, through `out` (exactly the
        keys to write)."""
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
                shape, dt = shapes[k]
                if (k, M) not in self._out:
                    self._out = {kk: v for kk, v in self._out.items() if kk[0] != k}   # one size kept per key
                    self._out[(k, M)] = torch.empty(shape, dtype=dt, device=e.device)
                t[k] = self._out[(k, M)]
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
        if M == 0:
            return t
        p = {k: (t[k].data_ptr() if k in t else None) for k in shapes}
        batch = nat.WhReplayBatch(p["obs"], p["next_obs"], p["xfrag"], p["next_xfrag"], p["state"], p["next_state"],
                                  p["actions"], p["rewards"], p["dones"], p["n"], p["idx_out"])
        e._call("wh_replay_gather", ctypes.byref(self._ring), self._filled, M, e._ptr(ix), e.seed,
                int(draw or 0) & 0xFFFFFFFFFFFFFFFF, ctypes.byref(batch), e.stream)
        return t
