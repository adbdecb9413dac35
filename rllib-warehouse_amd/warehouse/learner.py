"""A whole SAC learner update on the device (include/warehouse_amd.h, SAC LOSSES and ADAM;
csrc/sac_loss.h, csrc/adam.h).

`sac_losses` turns the learner's own logits at `obs` and the TD target into the three losses and their
d(loss)/d(logits) in one call; `DeviceAdam` steps up to 24 tensors in one launch; `SACLearner` strings
everything the package has into one `update(batch)`:

    pol_m, q1_m, q2_m = (torch.nn.Sequential(...).to("cuda") for _ in range(3))   # what weights_of accepts
    critic = SACCritic(policy, q1, q2, q1_target, q2_target, alpha=1.0, gamma=0.99)
    learner = SACLearner(pol_m, q1_m, q2_m, rollout_policy=policy, critic=critic,
                         log_alpha=torch.zeros(1, device="cuda"))
    batch = buf.sample(64, rows=True, fragments=True)
    out = learner.update(batch)                           # stats [6], td [M], y [M, NA]
    buf.update_priorities(batch["idx_out"], out["td"])

One host sync remains in the default update: wh_sac_td takes alpha by value, so `update` reads log_alpha
back (4 bytes) to set `critic.alpha`.  Everything else is enqueued on the current stream.

`SACLearner(..., sync_free=True)` removes it: the critic reads log_alpha on the device (wh_sac_td_la) and
Adam keeps its step count there (wh_adam_step_clock), so an update makes no host read and can be
captured once and replayed:

    learner = SACLearner(..., sync_free=True)
    batch = buf.sample(64, rows=True, fragments=True)     # the graph's inputs: these very tensors
    graph = learner.capture(batch, buf=buf)               # the learner is left as it was
    for _ in range(n):
        buf.sample(64, rows=True, fragments=True)         # the same M and flags: the same tensors
        graph.replay()                                    # update + update_priorities, one launch
        stats = graph.out["stats"]
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, List, Optional, Sequence

import torch

from . import _native as nat
from .batched import _check_out, require_device
from .policy import NUM_ACTIONS, weights_of
from .sac import SACCritic
from .train import KEYS, MLPTrainer, train_backward_many, train_forward_many

_buf: Dict[tuple, torch.Tensor] = {}
_work_bytes: Dict[tuple, int] = {}


def _own(device, k: str, shape, dt=torch.float32) -> torch.Tensor:
    """A buffer sac_losses owns: one size kept per device and name (as SACCritic._own)."""
    t = _buf.get((device, k))
    if t is None or tuple(t.shape) != tuple(shape):
        t = _buf[(device, k)] = torch.empty(shape, dtype=dt, device=device)
    return t


def loss_work_bytes(M: int, NA: int) -> int:
    """wh_sac_loss_query: the bytes of `work` for M samples of NA agents (asked once per size)."""
    if (M, NA) not in _work_bytes:
        n = ctypes.c_int64()
        nat.check(nat.lib().wh_sac_loss_query(M, NA, ctypes.byref(n)), "wh_sac_loss_query")
        _work_bytes[(M, NA)] = int(n.value)
    return _work_bytes[(M, NA)]


def _arg(t, what: str, shape, dtype, device) -> torch.Tensor:
    if not torch.is_tensor(t):
        raise ValueError(f"{what} must be a tensor")
    try:
        return _check_out(t, shape, dtype, device)
    except ValueError as e:
        raise ValueError(f"{what}: {e}") from None


def sac_losses(pi: torch.Tensor, q1: torch.Tensor, q2: Optional[torch.Tensor], y: torch.Tensor,
               actions: torch.Tensor, *, log_alpha: torch.Tensor, target_entropy: float,
               n: Optional[torch.Tensor] = None, weights: Optional[torch.Tensor] = None,
               scale: Optional[float] = None, out: Optional[Dict[str, torch.Tensor]] = None):
    """wh_sac_loss on the current stream, no host sync.

    pi, q1, q2: [M*NA, 9] float32 logits of the policy and the Q networks at `obs` (q2 None: no twin);
    y: [M, NA] float32, SACCritic's target; actions: [M, NA] int32; n: [M] int32 or None; weights: [M]
    float32 or None; log_alpha: a one-element float32 device tensor.  scale None = 1 / (M * NA).
    Returns {"dpi", "dq1", "dq2" (None without q2), "stats" [6]}: buffers this module owns, overwritten
    by the next call of the same size on the device -- or the caller's through `out` (any of the
    keys).  stats = (critic loss 1, critic loss 2, actor loss, alpha loss, d(alpha loss)/d(log_alpha),
    live rows).  ValueError for a wrong argument, before any native call."""
    if not torch.is_tensor(y) or y.dim() != 2:
        raise ValueError("y must be a [M, NA] tensor")
    M, NA = (int(s) for s in y.shape)
    if not 1 <= NA <= 16:
        raise ValueError(f"y: 1 .. 16 agents, got {NA}")
    dev, rows = y.device, M * NA
    _arg(y, "y", (M, NA), torch.float32, dev)
    _arg(pi, "pi", (rows, NUM_ACTIONS), torch.float32, dev)
    _arg(q1, "q1", (rows, NUM_ACTIONS), torch.float32, dev)
    if q2 is not None:
        _arg(q2, "q2", (rows, NUM_ACTIONS), torch.float32, dev)
    _arg(actions, "actions", (M, NA), torch.int32, dev)
    if n is not None:
        _arg(n, "n", (M,), torch.int32, dev)
    if weights is not None:
        _arg(weights, "weights", (M,), torch.float32, dev)
    if not torch.is_tensor(log_alpha) or log_alpha.numel() != 1:
        raise ValueError("log_alpha must be a one-element tensor")
    _arg(log_alpha, "log_alpha", log_alpha.shape, torch.float32, dev)
    keys = ("dpi", "dq1", "dq2", "stats") if q2 is not None else ("dpi", "dq1", "stats")
    shapes = dict(dpi=(rows, NUM_ACTIONS), dq1=(rows, NUM_ACTIONS), dq2=(rows, NUM_ACTIONS), stats=(6,))
    if out is not None:
        if any(k not in keys for k in out):
            raise ValueError(f"out: some of {keys}, got {sorted(out)}")
        for k, v in out.items():
            _arg(v, k, shapes[k], torch.float32, dev)
    require_device(dev)
    res = {k: (out[k] if out is not None and k in out else _own(dev, k, shapes[k])) for k in keys}
    res.setdefault("dq2", None)
    if M == 0:
        res["stats"].zero_()
        return res
    work = _own(dev, "work", (loss_work_bytes(M, NA),), torch.uint8)
    args = nat.WhSacLossArgs(pi.data_ptr(), q1.data_ptr(), nat.ptr(q2), y.data_ptr(), actions.data_ptr(), nat.ptr(n),
                             nat.ptr(weights), log_alpha.data_ptr(), float(target_entropy),
                             1.0 / rows if scale is None else float(scale), res["dpi"].data_ptr(),
                             res["dq1"].data_ptr(), nat.ptr(res["dq2"]), res["stats"].data_ptr(), work.data_ptr())
    with torch.cuda.device(dev):
        nat.check(nat.lib().wh_sac_loss(M, NA, ctypes.byref(args), nat.stream_of(dev)), "wh_sac_loss")
    return res


class DeviceAdam:
    """torch.optim.Adam (no amsgrad, no weight decay, not maximize) over up to 24 tensors, one launch per
    step (wh_adam_step).  The defaults are RLlib's SAC optimisers'.  `m` and `v` are torch tensors this
    object owns; the tensors are updated in place.

    `device_step=True` keeps the step count where the kernels run: the object owns a wh_adam_clock
    (`clock`, 56 bytes on the tensors' device) and `step()` calls wh_adam_step_clock, which advances it
    and steps the tensors with no host read -- what a captured stream needs, since a by-value table
    would repeat step t for ever.  Reading `t` then reads the clock back (a sync: for checkpoints)."""

    def __init__(self, tensors: Sequence[torch.Tensor], lr: float = 3e-4, betas=(0.9, 0.999), eps: float = 1e-8,
                 device_step: bool = False):
        tensors = [t.detach() if torch.is_tensor(t) else t for t in tensors]
        self.device = self._check(tensors, "tensors")
        self.tensors: List[torch.Tensor] = tensors
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.m = [torch.zeros_like(t) for t in tensors]
        self.v = [torch.zeros_like(t) for t in tensors]
        self.device_step = bool(device_step)
        self.clock: Optional[torch.Tensor] = None   # wh_adam_clock as 7 x 8 bytes: t, beta1^t, beta2^t, h
        if self.device_step:
            if not tensors:
                raise ValueError("DeviceAdam: device_step needs at least one tensor (the clock lives on its device)")
            self.clock = torch.zeros(ctypes.sizeof(nat.WhAdamClock) // 8, dtype=torch.float64, device=self.device)
        self._t = 0
        self._set_clock(0)
        self._segs = None   # (the gradients' addresses, the wh_adam_seg array built for them)

    def _set_clock(self, t: int, products=None) -> None:
        """The count, and with device_step the clock: beta^t given (a checkpoint's) or rebuilt on the
        host by t multiplications, as the tick forms them."""
        self._t = int(t)
        if self.clock is None:
            return
        c = nat.adam_clock(t, *self.betas) if products is None else \
            nat.WhAdamClock(int(t), float(products[0]), float(products[1]), nat.WhAdamHyper())
        self.clock.copy_(torch.frombuffer(bytearray(bytes(c)), dtype=torch.float64))

    def _read_clock(self) -> "nat.WhAdamClock":
        return nat.WhAdamClock.from_buffer_copy(self.clock.cpu().numpy().tobytes())

    @property
    def t(self) -> int:
        """Steps taken.  With device_step this reads the clock back from the device (a sync)."""
        return int(self._read_clock().t) if self.clock is not None else self._t

    @t.setter
    def t(self, value: int) -> None:
        self._set_clock(int(value))

    @staticmethod
    def _check(tensors, what: str):
        if len(tensors) > nat.WH_ADAM_MAX_SEGS:
            raise ValueError(f"{what}: at most {nat.WH_ADAM_MAX_SEGS} tensors in one launch, got {len(tensors)}")
        for i, t in enumerate(tensors):
            if not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_contiguous() or \
                    t.device != tensors[0].device:
                raise ValueError(f"{what}[{i}]: contiguous float32 tensors on one device")
        if tensors and torch.cuda.is_available() and tensors[0].device.type != "cuda":
            raise ValueError(f"{what}: on {tensors[0].device}, the kernel takes tensors on a HIP device")
        return require_device(tensors[0].device) if tensors else None

    def step(self, grads: Sequence[torch.Tensor]) -> None:
        """One Adam step from `grads` (one per tensor, its shape), on the current stream, no sync."""
        grads = list(grads)
        if len(grads) != len(self.tensors):
            raise ValueError(f"grads: {len(self.tensors)} tensors, got {len(grads)}")
        key = tuple(g.data_ptr() if torch.is_tensor(g) else None for g in grads)
        if self._segs is None or self._segs[0] != key:
            for i, (g, t) in enumerate(zip(grads, self.tensors)):
                if not torch.is_tensor(g) or g.dtype != torch.float32 or not g.is_contiguous() or \
                        g.device != t.device or g.numel() != t.numel():
                    raise ValueError(f"grads[{i}]: a contiguous float32 tensor of {t.numel()} elements on {t.device}")
            arr = (nat.WhAdamSeg * max(1, len(grads)))()
            for i, (t, m, v, g) in enumerate(zip(self.tensors, self.m, self.v, grads)):
                arr[i] = nat.WhAdamSeg(t.data_ptr(), m.data_ptr(), v.data_ptr(), g.data_ptr(), t.numel())
            self._segs = (key, arr)
        if self.clock is not None:   # the tick and the step, in stream order; the count stays on the device
            with torch.cuda.device(self.device):
                nat.check(nat.lib().wh_adam_step_clock(len(grads), self._segs[1], self.clock.data_ptr(), self.lr,
                                                       self.betas[0], self.betas[1], self.eps,
                                                       nat.stream_of(self.device)), "wh_adam_step_clock")
            return
        self._t += 1
        if not grads:
            return
        h = nat.adam_hyper(self.lr, self.betas[0], self.betas[1], self.eps, self._t)
        with torch.cuda.device(self.device):
            nat.check(nat.lib().wh_adam_step(len(grads), self._segs[1], ctypes.byref(h), nat.stream_of(self.device)),
                      "wh_adam_step")

    def state_dict(self) -> dict:
        """Copies of the step count, the moments and the hyper-parameters, for a checkpoint; with
        device_step also the clock's two running products ("beta_t"), read back from the device."""
        state = dict(step=self._t, lr=self.lr, betas=self.betas, eps=self.eps, m=[x.clone() for x in self.m],
                     v=[x.clone() for x in self.v])
        if self.clock is not None:
            c = self._read_clock()
            state.update(step=int(c.t), beta_t=(float(c.beta1_t), float(c.beta2_t)))
        return state

    def load_state_dict(self, state: dict) -> None:
        """A state of either form loads into either: one saved without the clock has its products
        rebuilt by `step` multiplications on the host."""
        if len(state["m"]) != len(self.m) or len(state["v"]) != len(self.v) or \
                any(a.shape != b.shape for a, b in zip(list(state["m"]) + list(state["v"]), self.m + self.v)):
            raise ValueError("load_state_dict: the moments do not match this optimiser's tensors")
        for dst, src in zip(self.m + self.v, list(state["m"]) + list(state["v"])):
            dst.copy_(src)
        self.lr, self.eps = float(state["lr"]), float(state["eps"])
        self.betas = (float(state["betas"][0]), float(state["betas"][1]))
        self._set_clock(int(state["step"]), state.get("beta_t"))


class SACLearner:
    """RLlib's discrete SAC learner step on the device, from what the package already has.

    `policy_module`, `q1_module`, `q2_module`: the Sequential(Linear, ReLU, Linear, ReLU, Linear)s that
    `weights_of` accepts, float32 on one HIP device (q2_module None with a critic without a twin): the
    master weights.  `rollout_policy`: the MLPPolicy the sampler runs, refreshed after every update.
    `critic`: the SACCritic whose q1 / q2 blobs mirror the two Q modules; its policy, when it is not
    `rollout_policy` itself (an f32 copy beside a bf16 sampler, say), is refreshed as well.  `log_alpha`: a one-element float32 device tensor, e.g. torch.zeros(1, device=...)
    for RLlib's initial alpha of 1; it is a parameter and is stepped in place.  target_entropy, lr and
    target_network_update_freq default to the experiment YAMLs'.  `fused_train`: True runs the modules'
    training passes in one launch per product for all of them (train_forward_many / train_backward_many),
    False one module after the other, None (default) takes the fused route when the modules have one
    shape and the batch has at most FUSED_TRAIN_MAX_ROWS agent rows; `update()` returns the same bytes
    either way.  `last_fused_train` says which route the last update took.  `sync_free`: False (default)
    reads log_alpha back once per update for the critic's by-value alpha and counts Adam's steps on the
    host; True hands log_alpha to the critic as a pointer (wh_sac_td_la) and uses
    DeviceAdam(device_step=True), so `update()` reads nothing back -- and `capture()` can record it."""

    # fused_train=None takes the fused route up to this many agent rows (M x NA): the largest batch at which
    # it measured faster by more than the spread of the sequential route's rounds.  SACLearner.update on
    # one MI355X, fused / sequential in us (profiles/mlp_train_multi_probe.txt): Small-4
    # 256 rows 273.6 / 306.8, 2,048 rows 303.8 / 430.2; Medium-8 512 rows 288.8 / 326.8, 4,096 rows 523.0 /
    # 697.8.  Nothing above 4,096 rows was measured, so nothing above takes the fused route unasked.
    FUSED_TRAIN_MAX_ROWS = 4096

    def __init__(self, policy_module, q1_module, q2_module, *, rollout_policy, critic: SACCritic,
                 log_alpha: torch.Tensor, target_entropy: float = 0.935, lr: float = 3e-4,
                 target_network_update_freq: int = 8000, fused_train: Optional[bool] = None,
                 sync_free: bool = False):
        if fused_train is not None and not isinstance(fused_train, bool):
            raise ValueError(f"SACLearner: fused_train is True, False or None, got {fused_train!r}")
        if not isinstance(sync_free, bool):
            raise ValueError(f"SACLearner: sync_free is True or False, got {sync_free!r}")
        self.sync_free = sync_free
        if not isinstance(critic, SACCritic):
            raise ValueError("SACLearner: critic is a SACCritic")
        if (q2_module is None) != (critic.q2 is None):
            raise ValueError("SACLearner: q2_module and the critic's q2 come together (both, or neither)")
        self.modules = [m for m in (policy_module, q1_module, q2_module) if m is not None]
        self.trainers = [MLPTrainer(m) for m in self.modules]
        self.device = self.trainers[0].device
        self.one_shape = all(t.dims == self.trainers[0].dims for t in self.trainers)
        if fused_train and not self.one_shape:
            raise ValueError("SACLearner: fused_train=True takes modules of one shape")
        self.fused_train = fused_train
        self.last_fused_train: Optional[bool] = None
        if any(t.device != self.device for t in self.trainers) or critic.device != self.device or \
                rollout_policy.device != self.device:
            raise ValueError("SACLearner: the modules, the rollout policy and the critic live on one device")
        if not torch.is_tensor(log_alpha) or log_alpha.numel() != 1 or log_alpha.dtype != torch.float32 or \
                log_alpha.device != self.device:
            raise ValueError(f"SACLearner: log_alpha is a one-element float32 tensor on {self.device}")
        if int(target_network_update_freq) < 1:
            raise ValueError("SACLearner: target_network_update_freq >= 1")
        self.rollout_policy, self.critic = rollout_policy, critic
        # the blobs that mirror a module: the rollout policy (and the critic's, when it is another object),
        # the critic's q1 / q2
        self.packed = [(rollout_policy, policy_module), (critic.q1, q1_module)]
        if critic.policy is not rollout_policy:
            self.packed.append((critic.policy, policy_module))
        if critic.q2 is not None:
            self.packed.append((critic.q2, q2_module))
        self.log_alpha = log_alpha.detach()
        self.target_entropy = float(target_entropy)
        self.target_network_update_freq = int(target_network_update_freq)
        self.params = [weights_of(m)[k] for m in self.modules for k in KEYS]
        self.adam = DeviceAdam(self.params + [self.log_alpha.view(1)], lr=lr, device_step=sync_free)
        self.updates = 0
        self.grads: Optional[List[torch.Tensor]] = None   # the gradients of the last update, in self.adam's order

    def use_fused_train(self, rows: int) -> bool:
        """Whether an update over `rows` agent rows runs the modules' training passes fused."""
        if self.fused_train is None:
            return self.one_shape and rows <= self.FUSED_TRAIN_MAX_ROWS
        return self.fused_train

    def update(self, batch: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """One learner step from a ReplayBuffer.sample(..., rows=True) dict (plus fragments=True when the
        critic's networks are bf16): critic.td, the three training forwards on batch["obs"], sac_losses
        (importance weights from batch["weights"] when the ring is prioritized), the three backwards (the
        forwards and the backwards each in one launch per product for all modules on the fused route), ONE
        Adam launch over the 18 parameter tensors and log_alpha (whose gradient is stats[4], in place),
        the repack of the rollout policy and the critic's networks, and every target_network_update_freq
        updates critic.sync_targets().  Returns {"stats" [6], "td" [M], "y" [M, NA]}; the caller does
        buf.update_priorities(batch["idx_out"], out["td"]).  Reads log_alpha back once (the only sync);
        with sync_free, not even that."""
        out = self._launches(batch)
        self.updates += 1
        if self.updates % self.target_network_update_freq == 0:
            self.critic.sync_targets()
        return out

    def _launches(self, batch: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """update() up to the repack: everything whose launches are the same from one update to the next
        (what capture() records); the count and the periodic target sync are update()'s and replay()'s."""
        if "obs" not in batch:
            raise ValueError("SACLearner: the batch holds no obs rows (sample(rows=True))")
        if self.sync_free:
            td = self.critic.td(batch, log_alpha=self.log_alpha)
        else:
            self.critic.alpha = math.exp(float(self.log_alpha.item()))
            td = self.critic.td(batch)
        M, NA = td["y"].shape
        obs = batch["obs"].view(M * NA, -1)
        fused = self.last_fused_train = self.use_fused_train(M * NA)
        if fused:
            logits = train_forward_many(self.trainers, obs)
        else:
            logits = [t.forward(obs) for t in self.trainers]
        loss = sac_losses(logits[0], logits[1], logits[2] if len(logits) > 2 else None, td["y"], batch["actions"],
                          log_alpha=self.log_alpha, target_entropy=self.target_entropy, n=batch.get("n"),
                          weights=batch.get("weights"))
        dz = [loss[k] for _, k in zip(self.trainers, ("dpi", "dq1", "dq2"))]
        if fused:
            per_net = train_backward_many(self.trainers, dz)
        else:
            per_net = [t.backward(d) for t, d in zip(self.trainers, dz)]
        grads = [g[kk] for g in per_net for kk in KEYS]
        self.grads = grads + [loss["stats"][4:5]]
        self.adam.step(self.grads)
        for net, m in self.packed:
            net.load_weights(weights_of(m))
        return dict(stats=loss["stats"], td=td["td"], y=td["y"])

    # ------------------------------------------------------------------ capture and replay
    def _nets(self) -> list:
        """Every network whose blob an update writes: the repacked ones and the targets."""
        return [net for net, _ in self.packed] + [n for n in (self.critic.q1_target, self.critic.q2_target) if n is not None]

    def _written(self) -> List[torch.Tensor]:
        """Every device tensor an update writes: the parameters and log_alpha, Adam's moments and clock, and
        every packed blob, the targets included."""
        return self.adam.tensors + self.adam.m + self.adam.v + [self.adam.clock] + [n.packed for n in self._nets()]

    def capture(self, batch: Dict[str, torch.Tensor], buf=None) -> "CapturedUpdate":
        """Record one update(batch) -- followed, with `buf`, by buf.update_priorities(batch["idx_out"],
        out["td"]) -- as a graph (torch.cuda.graph) and return a CapturedUpdate: `replay()` runs it, `out`
        is the dict update() would return (the learner's own tensors, overwritten by every replay).

        Needs sync_free=True (ValueError otherwise): a captured by-value alpha or Adam table would be
        frozen.  The learner leaves capture() in the state it entered it: everything an update writes is
        saved, one eager update(batch) warms up (buffer allocation, the pack table's upload, torch's lazy
        initialisation -- none of which may happen inside a capture), the state is restored, the update is
        recorded (recording runs nothing), and `updates` is as before.  The fused or sequential choices
        (use_fused_train, SACCritic.use_fused) are made here, once, for this batch's size.  The recorded
        graph is one chain of launches on one stream.

        The batch's tensors are the graph's inputs, by address: keep sampling into them --
        buf.sample(M, ...) with the same M and flags, or out= -- before each replay().  The exception is
        "weights": a prioritized sample() computes a fresh tensor each time, so the graph reads a tensor
        of its own and replay(batch) copies the batch's weights into it first."""
        if not self.sync_free:
            raise ValueError("SACLearner.capture: needs sync_free=True (a captured update must read alpha and "
                             "Adam's step count on the device)")
        if buf is not None and not getattr(buf, "prioritized", False):
            raise ValueError("SACLearner.capture: buf is the prioritized ReplayBuffer whose priorities the update sets")
        if buf is not None and "idx_out" not in batch:
            raise ValueError("SACLearner.capture: with buf, the batch holds idx_out")
        batch = dict(batch)
        if batch.get("weights") is not None:
            batch["weights"] = batch["weights"].clone()
        nets = self._nets()
        written = self._written() + ([] if buf is None else [buf.prio_leaf, buf.prio_node, buf.prio_max_q])
        saved = [t.clone() for t in written]
        updates, host_weights = self.updates, [n.weights for n in nets]
        warm = self.update(batch)                            # the warm-up, eager
        if buf is not None:
            buf.update_priorities(batch["idx_out"], warm["td"])
        for t, s in zip(written, saved):
            t.copy_(s)
        self.updates = updates
        torch.cuda.synchronize(self.device)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):                        # recording runs nothing: the device state stays restored
            out = self._launches(batch)
            if buf is not None:
                buf.update_priorities(batch["idx_out"], out["td"])
        for n, w in zip(nets, host_weights):                 # (the host copies a repack or a target sync drops)
            n.weights = w
        keep = [t for tr in self.trainers for t in tr._buf.values()] + list(self.critic._buf.values()) + \
            [t for (dev, _), t in _buf.items() if dev == self.device]
        return CapturedUpdate(self, graph, batch, out, keep)


class CapturedUpdate:
    """SACLearner.capture's result.  `out`: {"stats" [6], "td" [M], "y" [M, NA]}, the learner's tensors, as
    the last replay() left them.  `replay()` launches the recorded update on the current stream, counts
    it in `learner.updates` and, every target_network_update_freq updates, calls critic.sync_targets()
    after the launch (eagerly: stream order puts it behind the update, and the count is the host's)."""

    def __init__(self, learner: SACLearner, graph, batch: Dict[str, torch.Tensor], out: Dict[str, torch.Tensor], keep):
        self.learner, self.graph, self.batch, self.out = learner, graph, batch, out
        self._keep = keep   # every buffer the graph's launches address, alive as long as the graph is
        self._addresses = {k: v.data_ptr() for k, v in batch.items() if torch.is_tensor(v) and k != "weights"}

    def replay(self, batch: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """One update from what the captured batch's tensors hold now.  `batch`, when given, must be those
        very tensors (ValueError for another key set or address): it is there to be checked, and for its
        "weights", which are copied into the graph's own tensor."""
        if batch is not None:
            got = {k: v.data_ptr() for k, v in batch.items() if torch.is_tensor(v) and k != "weights"}
            if got != self._addresses:
                diff = sorted(k for k in set(got) | set(self._addresses) if got.get(k) != self._addresses.get(k))
                raise ValueError(f"CapturedUpdate.replay: the batch is not the captured one (differs in {diff}); "
                                 "sample into the captured tensors")
            if ("weights" in batch) != ("weights" in self.batch):
                raise ValueError("CapturedUpdate.replay: the captured batch and this one differ in 'weights'")
            if "weights" in batch:
                self.batch["weights"].copy_(batch["weights"], non_blocking=True)
        self.graph.replay()
        ln = self.learner
        ln.updates += 1
        if ln.updates % ln.target_network_update_freq == 0:
            ln.critic.sync_targets()
        return self.out
