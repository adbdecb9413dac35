"""The SAC policy network on the device (wh_mlp_forward): `trainer.compute_action(obs)` of
scripts/rollout.py:72 for every agent row of a batch, so a trained-policy rollout stays on the
GPU next to the simulator.

Architecture = the policy_model of scripts/experiments/warehouse-{small,medium,large}-sac/*.yaml:
flat observation row (9R+1) -> Linear -> ReLU -> Linear -> ReLU -> Linear -> 9 action logits, hidden
sizes [256,256] / [512,512] / [1024,256].  Weights come in torch nn.Linear layout ([out, in]); no
checkpoint ships with the reference, so `MLPPolicy(variant)` initialises them like nn.Linear's
default (U(-1/sqrt(fan_in), 1/sqrt(fan_in))) from a seed.

precision="bf16" (default, fast): bf16 MFMA, f32 accumulation, activations rounded to bf16 between
layers.  precision="f32": exact f32 on v_mfma_f32_32x32x2_f32 (an fmaf chain per output), i.e. the
reference's TF fp32 policy up to summation order -- about 6x slower.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import numpy as np
import torch

from . import _native as nat
from ._geometry import GEOMETRY
from .batched import require_device

HIDDEN = {"small": (256, 256), "medium": (512, 512), "large": (1024, 256)}
NUM_ACTIONS = 9
PRECISIONS = {"bf16": nat.WH_MLP_BF16, "f32": nat.WH_MLP_F32}


def init_weights(in_dim: int, hidden0: int, hidden1: int, seed: int = 0) -> Dict[str, np.ndarray]:
    """nn.Linear-style uniform init, float32, [out, in] layout."""
    rng = np.random.RandomState(seed)
    out = {}
    for name, (fo, fi) in (("0", (hidden0, in_dim)), ("1", (hidden1, hidden0)), ("2", (NUM_ACTIONS, hidden1))):
        bound = 1.0 / np.sqrt(fi)
        out["w" + name] = rng.uniform(-bound, bound, size=(fo, fi)).astype(np.float32)
        out["b" + name] = rng.uniform(-bound, bound, size=(fo,)).astype(np.float32)
    return out


class MLPPolicy:
    def __init__(self, variant: str = "medium", weights: Optional[Dict[str, object]] = None, *,
                 seed: int = 0, device=None, precision: str = "bf16"):
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(PRECISIONS)}")
        R = GEOMETRY[variant]["R"]
        self.in_dim = 9 * R + 1
        self.hidden = HIDDEN[variant]
        self.precision = precision
        self.device = require_device(device)
        self.desc = nat.WhMlpDesc(self.in_dim, self.hidden[0], self.hidden[1], NUM_ACTIONS, PRECISIONS[precision])
        nbytes = ctypes.c_int64()
        nat.check(nat.lib().wh_mlp_query(ctypes.byref(self.desc), ctypes.byref(nbytes)), "wh_mlp_query")
        if weights is None:
            weights = init_weights(self.in_dim, *self.hidden, seed=seed)
        self.weights = {k: np.ascontiguousarray(np.asarray(v.cpu() if torch.is_tensor(v) else v, np.float32))
                        for k, v in weights.items()}
        w = self.weights
        shapes = dict(w0=(self.hidden[0], self.in_dim), b0=(self.hidden[0],), w1=(self.hidden[1], self.hidden[0]),
                      b1=(self.hidden[1],), w2=(NUM_ACTIONS, self.hidden[1]), b2=(NUM_ACTIONS,))
        for k, shp in shapes.items():
            if w[k].shape != shp:
                raise ValueError(f"{k}: expected {shp}, got {w[k].shape}")
        self.packed = torch.empty(int(nbytes.value), dtype=torch.uint8, device=self.device)
        fp = ctypes.POINTER(ctypes.c_float)
        args = [w[k].ctypes.data_as(fp) for k in ("w0", "b0", "w1", "b1", "w2", "b2")]
        with torch.cuda.device(self.device):
            nat.check(nat.lib().wh_mlp_pack(ctypes.byref(self.desc), *args, self.packed.data_ptr()), "wh_mlp_pack")
        self._step = 0

    def _shapes(self) -> Dict[str, tuple]:
        return dict(w0=(self.hidden[0], self.in_dim), b0=(self.hidden[0],), w1=(self.hidden[1], self.hidden[0]),
                    b1=(self.hidden[1],), w2=(NUM_ACTIONS, self.hidden[1]), b2=(NUM_ACTIONS,))

    def load_weights(self, weights: Dict[str, object]) -> None:
        """Repack this network from `weights` (keys w0 b0 w1 b1 w2 b2, nn.Linear layout).

        When every value is a contiguous float32 torch tensor on `self.device`, the blob is repacked
        by wh_mlp_pack_device on the current stream: no copy of the weights to the host and no
        synchronisation, so a learner refreshes its rollout policy (or a Q network) between two
        launches.  `self.weights` then becomes None: the host copy the constructor kept would be
        stale, and fetching a fresh one would be the very sync this avoids.  (The first device
        repack of a shape uploads a small table and must not happen inside a stream capture.)
        Anything else -- numpy arrays, host tensors, another dtype or device -- takes the
        constructor's host path (wh_mlp_pack, synchronous) and refreshes `self.weights`.  Shapes are
        checked as the constructor checks them."""
        shapes = self._shapes()
        on_device = all(torch.is_tensor(weights[k]) and weights[k].device == self.device and
                        weights[k].dtype == torch.float32 and weights[k].is_contiguous() for k in shapes)
        fp = ctypes.POINTER(ctypes.c_float)
        if on_device:
            for k, shp in shapes.items():
                if tuple(weights[k].shape) != shp:
                    raise ValueError(f"{k}: expected {shp}, got {tuple(weights[k].shape)}")
            args = [weights[k].data_ptr() for k in shapes]
            nat.check(nat.lib().wh_mlp_pack_device(ctypes.byref(self.desc), *args, self.packed.data_ptr(),
                                                   nat.stream_of(self.device)), "wh_mlp_pack_device")
            self.weights = None
            return
        w = {k: np.ascontiguousarray(np.asarray(v.detach().cpu() if torch.is_tensor(v) else v, np.float32))
             for k, v in weights.items()}
        for k, shp in shapes.items():
            if w[k].shape != shp:
                raise ValueError(f"{k}: expected {shp}, got {w[k].shape}")
        args = [w[k].ctypes.data_as(fp) for k in shapes]
        with torch.cuda.device(self.device):
            nat.check(nat.lib().wh_mlp_pack(ctypes.byref(self.desc), *args, self.packed.data_ptr()), "wh_mlp_pack")
        self.weights = w

    def copy_from(self, other: "MLPPolicy") -> None:
        """This network's packed blob <- `other`'s, a device-to-device copy on the current stream:
        the YAMLs' target update (tau: 1.0, every target_network_update_freq steps).  Both must have
        the same variant shape and precision (blobs are specific to both)."""
        same = (self.in_dim, self.hidden, self.precision) == (other.in_dim, other.hidden, other.precision)
        if not same or self.packed.numel() != other.packed.numel():
            raise ValueError("copy_from: the two networks differ in variant or precision")
        self.packed.copy_(other.packed, non_blocking=True)
        self.weights = other.weights

    def forward(self, obs: torch.Tensor, *, explore: bool = False, seed: int = 0, step: Optional[int] = None,
                actions: Optional[torch.Tensor] = None, logits: Optional[torch.Tensor] = None):
        """obs [..., 9R+1] f32 device rows -> (actions [...] int32, logits [..., 9] f32 or None).
        `logits` / `actions` may be passed as output buffers; pass logits=True for a fresh one."""
        lead = obs.shape[:-1]
        if obs.shape[-1] != self.in_dim or obs.dtype != torch.float32 or not obs.is_contiguous():
            raise ValueError(f"obs must be contiguous float32 [..., {self.in_dim}]")
        rows = int(np.prod(lead)) if lead else 1
        if actions is None:
            actions = torch.empty(lead, dtype=torch.int32, device=self.device)
        if logits is True:
            logits = torch.empty((*lead, NUM_ACTIONS), dtype=torch.float32, device=self.device)
        if step is None:
            step, self._step = self._step, self._step + 1
        nat.check(nat.lib().wh_mlp_forward(ctypes.byref(self.desc), self.packed.data_ptr(), rows, obs.data_ptr(),
                                           nat.ptr(logits if logits is not None and logits is not False else None),
                                           actions.data_ptr(), int(bool(explore)), int(seed), int(step) & 0xFFFFFFFF,
                                           nat.stream_of(self.device)), "wh_mlp_forward")
        return actions, (logits if torch.is_tensor(logits) else None)

    __call__ = forward

    def forward_x(self, xfrag: torch.Tensor, rows: int, *, explore: bool = False, seed: int = 0,
                  step: Optional[int] = None, actions: Optional[torch.Tensor] = None,
                  logits: Optional[torch.Tensor] = None):
        """forward() on BatchedWarehouse.observe_x()'s fragment-order operand (rows = B x NA agent
        rows; bf16 precision only): the same actions/logits as forward() on the f32 rows."""
        if self.precision != "bf16":
            raise ValueError("forward_x needs precision='bf16'")
        if actions is None:
            actions = torch.empty(rows, dtype=torch.int32, device=self.device)
        if logits is True:
            logits = torch.empty((rows, NUM_ACTIONS), dtype=torch.float32, device=self.device)
        if step is None:
            step, self._step = self._step, self._step + 1
        nat.check(nat.lib().wh_mlp_forward_x(ctypes.byref(self.desc), self.packed.data_ptr(), int(rows),
                                             xfrag.data_ptr(),
                                             nat.ptr(logits if logits is not None and logits is not False else None),
                                             actions.data_ptr(), int(bool(explore)), int(seed), int(step) & 0xFFFFFFFF,
                                             nat.stream_of(self.device)), "wh_mlp_forward_x")
        return actions, (logits if torch.is_tensor(logits) else None)


MAX_JOBS = nat.WH_MLP_MAX_JOBS


def forward_many(jobs):
    """Several networks of one shape, precision and device in ONE launch (wh_mlp_forward_multi): the
    workgroups of the launch are shared out among the jobs, so small forwards that would each fill a
    few CUs one after the other run side by side.  Every job writes byte for byte what
    `net.forward` / `net.forward_x` writes for the same arguments.

    `jobs`: up to MAX_JOBS dicts with
        net      the MLPPolicy
        obs      [..., 9R+1] contiguous f32 device rows, or
        xfrag    observe_x()'s fragment-order operand, with `rows` (bf16 networks only)
        logits   an output buffer, or True for a fresh one (default: none)
        actions  an output buffer, or True for a fresh one; when omitted, a fresh one unless logits
                 are asked for -- then no actions are computed (NULL goes to the ABI, no scratch)
        explore, seed, step   as forward(); step=None takes the network's own counter
    Returns one (actions, logits) pair per job (None for an output the job did not ask for)."""
    jobs = list(jobs)
    if len(jobs) > MAX_JOBS:
        raise ValueError(f"forward_many: at most {MAX_JOBS} jobs in one launch, got {len(jobs)}")
    if not jobs:
        return []
    nets = []
    for j in jobs:
        unknown = set(j) - {"net", "obs", "xfrag", "rows", "logits", "actions", "explore", "seed", "step"}
        if unknown:
            raise ValueError(f"forward_many: unknown job keys {sorted(unknown)}")
        if not isinstance(j.get("net"), MLPPolicy):
            raise ValueError("forward_many: every job names its MLPPolicy as 'net'")
        nets.append(j["net"])
    n0 = nets[0]
    for n in nets[1:]:
        if (n.in_dim, n.hidden, n.precision) != (n0.in_dim, n0.hidden, n0.precision) or n.device != n0.device:
            raise ValueError("forward_many: the networks of one launch share shape, precision and device")
    table = (nat.WhMlpJob * len(jobs))()
    results = []
    for t, j, net in zip(table, jobs, nets):
        obs, xfrag = j.get("obs"), j.get("xfrag")
        if (obs is None) == (xfrag is None):
            raise ValueError("forward_many: a job reads either 'obs' or 'xfrag'")
        if obs is not None:
            if obs.shape[-1] != net.in_dim or obs.dtype != torch.float32 or not obs.is_contiguous():
                raise ValueError(f"obs must be contiguous float32 [..., {net.in_dim}]")
            lead = tuple(obs.shape[:-1])
            rows = int(np.prod(lead)) if lead else 1
        else:
            if net.precision != "bf16":
                raise ValueError("an 'xfrag' job needs precision='bf16'")
            if "rows" not in j:
                raise ValueError("forward_many: an 'xfrag' job states its 'rows'")
            rows = int(j["rows"])
            lead = (rows,)
        logits, actions = j.get("logits"), j.get("actions")
        if logits is True:
            logits = torch.empty((*lead, NUM_ACTIONS), dtype=torch.float32, device=net.device)
        elif logits is False:
            logits = None
        if actions is True or (actions is None and logits is None):
            actions = torch.empty(lead, dtype=torch.int32, device=net.device)
        elif actions is False:
            actions = None
        t.packed, t.rows = net.packed.data_ptr(), rows
        t.obs, t.xfrag = nat.ptr(obs), nat.ptr(xfrag)
        t.logits, t.actions = nat.ptr(logits), nat.ptr(actions)
        t.explore, t.seed = int(bool(j.get("explore", False))), int(j.get("seed", 0))
        if j.get("step") is not None:
            t.step = int(j["step"]) & 0xFFFFFFFF
        results.append((actions, logits))
    # every job is valid: only now do the networks' own counters move (a refused call leaves them alone)
    for t, j, net in zip(table, jobs, nets):
        if j.get("step") is None:
            t.step, net._step = net._step & 0xFFFFFFFF, net._step + 1
    nat.check(nat.lib().wh_mlp_forward_multi(ctypes.byref(n0.desc), len(jobs), table, nat.stream_of(n0.device)),
              "wh_mlp_forward_multi")
    return results


def weights_of(module) -> Dict[str, torch.Tensor]:
    """The six parameter tensors of a torch.nn.Sequential(Linear, ReLU, Linear, ReLU, Linear) under
    the keys MLPPolicy takes, detached and without copies (they share the module's storage): what
    `policy.load_weights(weights_of(module))` packs after an optimiser step."""
    linears = [m for m in module if isinstance(m, torch.nn.Linear)]
    acts = [m for m in module if not isinstance(m, torch.nn.Linear)]
    if len(linears) != 3 or len(module) != 5 or not all(isinstance(m, torch.nn.ReLU) for m in acts) or \
            any(m.bias is None for m in linears):
        raise ValueError("weights_of: expected Sequential(Linear, ReLU, Linear, ReLU, Linear) with biases")
    out = {}
    for i, m in enumerate(linears):
        out[f"w{i}"] = m.weight.detach()
        out[f"b{i}"] = m.bias.detach()
    return out


def policy_rollout(env, net: MLPPolicy, steps: int, *, explore: bool = False, seed: int = 0,
                   first_step: int = 0, record=None, operand: str = "auto"):
    """scripts/rollout.py's loop (compute_action per agent -> env.step, until done) for every env
    of a BatchedWarehouse, on the device: per step one network forward over all B x NA observation
    rows, then the step (step + auto-reset + the next rows).  operand="fragments" (the default for
    bf16 networks) hands the rows to the network as its layer-0 operand (wh_vector_step_x writes
    it, wh_mlp_forward_x reads it: the same actions, no f32 rows materialised); "rows" uses the
    float32 observation rows (wh_vector_step).  `record`, if given, is called as record(step, actions, rewards,
    dones) with env-owned device tensors.  Returns the last step's observations (the fragment
    buffer or the obs tensor)."""
    if operand == "auto":
        operand = "fragments" if net.precision == "bf16" else "rows"
    if operand not in ("fragments", "rows"):
        raise ValueError("operand must be 'auto', 'fragments' or 'rows'")
    B, NA = env.B, env.agent_slots
    acts = torch.empty((B, NA), dtype=torch.int32, device=env.device)
    frag = operand == "fragments"
    obs = env.observe_x() if frag else env.observe()
    for s in range(steps):
        if frag:
            net.forward_x(obs, B * NA, explore=explore, seed=seed, step=first_step + s, actions=acts.view(-1))
            obs, rew, done = env.vector_step_x(acts, autoreset=True)   # step + the next operand
        else:
            net(obs.view(B * NA, -1), explore=explore, seed=seed, step=first_step + s, actions=acts.view(-1))
            obs, rew, done = env.vector_step(acts, autoreset=True, observe=True)
        if record is not None:
            record(s, acts, rew, done)
    return obs


def policy_collect(buf, net: MLPPolicy, steps: int, *, explore: bool = True, seed: int = 0, first_step: int = 0):
    """policy_rollout's loop recording into a ReplayBuffer: per step one network forward over all
    B x NA rows, then buf.step -- the recorded step and the next rows.  A bf16 network reads the
    fragment operand (`buf.step(acts, operand="fragments")`), an f32 network the float32 rows.  The
    trajectory, the actions and the ring are those of policy_rollout with a recorder.  Returns the
    last step's observations (the fragment buffer or the obs tensor)."""
    env = buf.env
    B, NA = env.B, env.agent_slots
    acts = torch.empty((B, NA), dtype=torch.int32, device=env.device)
    frag = net.precision == "bf16"
    obs = env.observe_x() if frag else env.observe()
    for s in range(steps):
        if frag:
            net.forward_x(obs, B * NA, explore=explore, seed=seed, step=first_step + s, actions=acts.view(-1))
            obs, _, _ = buf.step(acts, operand="fragments")
        else:
            net(obs.view(B * NA, -1), explore=explore, seed=seed, step=first_step + s, actions=acts.view(-1))
            obs, _, _ = buf.step(acts)
    return obs
