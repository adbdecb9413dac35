"""The policy / Q network's forward and backward for a learner, on the device in exact f32
(include/warehouse_amd.h, MLP TRAINING; csrc/mlp_train.h).

A learner keeps its networks as `torch.nn.Sequential(Linear, ReLU, Linear, ReLU, Linear)` -- what
`weights_of` accepts and `MLPPolicy.load_weights` packs.  The kernels here read those parameters where
they lie (nn.Linear layout, f32, no blob) and write gradients in the same layout, so the learner needs
no second, torch copy of the forward for autograd to see:

    logits = warehouse.mlp_logits(q_module, batch_obs)        # drop-in for q_module(batch_obs)
    loss = critic_loss(logits, y)                             # torch: losses stay the learner's
    loss.backward()                                           # wh_mlp_backward fills param.grad
    optimiser.step()                                          # torch
    q.load_weights(weights_of(q_module))                      # the device packer, same stream

`mlp_logits` is a torch.autograd.Function over the six parameters; `MLPTrainer` is the same pair of
calls without autograd, on buffers it owns; `train_forward_many` / `train_backward_many` run up to four
trainers of one shape in one launch per product (wh_mlp_train_forward_multi / wh_mlp_backward_multi),
with the bytes of the trainers' own calls.  Losses, d(loss)/d(logits) and the optimiser step on the
device are warehouse/learner.py's.
No gradient with respect to the observations is produced, and there is no double backward.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Tuple

import torch
from torch.autograd.function import once_differentiable

from . import _native as nat
from .batched import _check_out, require_device
from .policy import HIDDEN, NUM_ACTIONS, weights_of
from ._geometry import GEOMETRY

KEYS = ("w0", "b0", "w1", "b1", "w2", "b2")
# (in_dim, hidden0, hidden1) of the three variants' policy_model / Q_model
SHAPES = {(9 * GEOMETRY[v]["R"] + 1, *HIDDEN[v]): v for v in HIDDEN}


def _network(module) -> Tuple[Dict[str, torch.Tensor], Tuple[int, int, int]]:
    """The module's six parameters (weights_of: detached, sharing storage) and its (in, h0, h1), after
    every check that needs no device: the Sequential's form, f32, contiguity, one device, a variant's
    shape.  ValueError otherwise."""
    w = weights_of(module)
    dev = w["w0"].device
    for k in KEYS:
        t = w[k]
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{k}: the parameters are contiguous float32 tensors on one device "
                             f"(got {t.dtype}, contiguous={t.is_contiguous()}, {t.device})")
    h0, in_dim = (int(s) for s in w["w0"].shape)
    h1 = int(w["w1"].shape[0])
    dims = (in_dim, h0, h1)
    shapes = dict(w0=(h0, in_dim), b0=(h0,), w1=(h1, h0), b1=(h1,), w2=(NUM_ACTIONS, h1), b2=(NUM_ACTIONS,))
    if dims not in SHAPES or any(tuple(w[k].shape) != shapes[k] for k in KEYS):
        raise ValueError(f"the network {[tuple(w[k].shape) for k in KEYS]} is no variant's: expected "
                         f"(in, hidden0, hidden1) among {sorted(SHAPES)} and {NUM_ACTIONS} outputs")
    return w, dims


def _device_of(w) -> torch.device:
    """The HIP device the parameters live on.  Where there is a GPU, parameters elsewhere (the CPU) are a
    wrong argument: ValueError.  Where there is none, the package's usual RuntimeError (no CPU fallback)."""
    dev = w["w0"].device
    if torch.cuda.is_available() and dev.type != "cuda":
        raise ValueError(f"the parameters are on {dev}: the kernels take a network on a HIP device")
    return require_device(dev)


def _check_rows(t, what: str, width: int, device, dims=2) -> int:
    if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != dims or t.shape[-1] != width or \
            not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous float32 [rows, {width}] tensor")
    if t.device != device:
        raise ValueError(f"{what} must be on the network's device {device}, got {t.device}")
    if t.shape[0] > nat.WH_MLP_TRAIN_MAX_ROWS:
        raise ValueError(f"{what}: at most {nat.WH_MLP_TRAIN_MAX_ROWS} rows")
    return int(t.shape[0])


def _check_obs(obs, dims, device) -> int:
    rows = _check_rows(obs, "obs", dims[0], device)
    if obs.requires_grad:
        raise ValueError("obs.requires_grad: no gradient with respect to the observations is produced")
    return rows


def _desc(dims) -> nat.WhMlpDesc:
    return nat.WhMlpDesc(dims[0], dims[1], dims[2], NUM_ACTIONS, nat.WH_MLP_F32)


_work_bytes: Dict[tuple, int] = {}


def work_bytes(dims, rows: int) -> int:
    """wh_mlp_train_query: the bytes of `work` for a backward over `rows` rows (asked once per size)."""
    key = (tuple(dims), int(rows))
    if key not in _work_bytes:
        n = ctypes.c_int64()
        desc = _desc(dims)
        nat.check(nat.lib().wh_mlp_train_query(ctypes.byref(desc), int(rows), ctypes.byref(n)), "wh_mlp_train_query")
        _work_bytes[key] = int(n.value)
    return _work_bytes[key]


def _struct(w) -> nat.WhMlpWeights:
    return nat.WhMlpWeights(*[w[k].data_ptr() for k in KEYS])


_dummy: Dict[torch.device, torch.Tensor] = {}


def _ptr(t: torch.Tensor) -> int:
    """data_ptr(), or for a tensor of no rows (whose data_ptr() is NULL, which the ABI refuses even for
    rows == 0) the address of 16 bytes nobody reads."""
    if t.numel():
        return t.data_ptr()
    if t.device not in _dummy:
        _dummy[t.device] = torch.zeros(16, dtype=torch.uint8, device=t.device)
    return _dummy[t.device].data_ptr()


def _run_forward(dims, w, obs, h0, h1, logits) -> None:
    desc, ws = _desc(dims), _struct(w)
    with torch.cuda.device(obs.device):
        nat.check(nat.lib().wh_mlp_train_forward(ctypes.byref(desc), ctypes.byref(ws), obs.shape[0], _ptr(obs),
                                                 _ptr(h0), _ptr(h1), _ptr(logits),
                                                 nat.stream_of(obs.device)), "wh_mlp_train_forward")


def _run_backward(dims, w, obs, h0, h1, dlogits, grads, work) -> None:
    desc, ws, gs = _desc(dims), _struct(w), _struct(grads)
    with torch.cuda.device(obs.device):
        nat.check(nat.lib().wh_mlp_backward(ctypes.byref(desc), ctypes.byref(ws), obs.shape[0], _ptr(obs),
                                            _ptr(h0), _ptr(h1), _ptr(dlogits), ctypes.byref(gs),
                                            work.data_ptr(), nat.stream_of(obs.device)), "wh_mlp_backward")


class _MlpLogits(torch.autograd.Function):
    @staticmethod
    def forward(ctx, obs, dims, *params):
        rows, dev = obs.shape[0], obs.device
        w = dict(zip(KEYS, params))
        h0 = torch.empty((rows, dims[1]), dtype=torch.float32, device=dev)
        h1 = torch.empty((rows, dims[2]), dtype=torch.float32, device=dev)
        logits = torch.empty((rows, NUM_ACTIONS), dtype=torch.float32, device=dev)
        _run_forward(dims, w, obs, h0, h1, logits)
        ctx.dims = dims
        ctx.save_for_backward(obs, h0, h1, *params)
        return logits

    @staticmethod
    @once_differentiable
    def backward(ctx, dlogits):
        obs, h0, h1, *params = ctx.saved_tensors
        dims, dev = ctx.dims, obs.device
        if dlogits.dtype != torch.float32 or dlogits.device != dev:
            raise ValueError("mlp_logits: the gradient of the logits is a float32 tensor on the network's device")
        dz = dlogits.contiguous()                   # (e.g. sum()'s expanded gradient has stride 0)
        grads = {k: torch.empty_like(p) for k, p in zip(KEYS, params)}
        work = torch.empty(work_bytes(dims, obs.shape[0]), dtype=torch.uint8, device=dev)
        _run_backward(dims, dict(zip(KEYS, params)), obs, h0, h1, dz, grads, work)
        # (one backward computes all six; a parameter that asks for none gets None)
        return (None, None) + tuple(grads[k] if need else None for k, need in zip(KEYS, ctx.needs_input_grad[2:]))


def mlp_logits(module, obs: torch.Tensor) -> torch.Tensor:
    """`module(obs)` on the device kernels, differentiable with respect to the module's six parameters.

    `module`: the Sequential(Linear, ReLU, Linear, ReLU, Linear) that `weights_of` accepts, of a
    variant's shape, its parameters contiguous float32 on one HIP device.  `obs`: [rows, in_dim],
    contiguous float32 on that device, not requiring grad.  Returns logits [rows, 9] (exact f32: a
    float32 reference up to summation order).  `loss.backward()` runs wh_mlp_backward on the then
    current stream and accumulates into `param.grad` as autograd does, so a torch optimiser steps as
    usual.  ValueError for a bad argument (before any native call); the package's RuntimeError when
    there is no HIP device."""
    w, dims = _network(module)
    _check_obs(obs, dims, w["w0"].device)
    _device_of(w)
    linears = [m for m in module if isinstance(m, torch.nn.Linear)]
    params = [p for m in linears for p in (m.weight, m.bias)]     # KEYS order
    return _MlpLogits.apply(obs, dims, *params)


class MLPTrainer:
    """The explicit form of `mlp_logits`, without autograd: `forward(obs)` keeps what `backward(dlogits)`
    needs.  It owns h0 / h1 / work, the logits and the six gradient tensors (one size kept of each, as
    SACCritic does), so a returned tensor is overwritten by the next call unless `out` was given.  The
    module's parameters are read where they lie at every call: an optimiser step in between is seen."""

    def __init__(self, module):
        w, self.dims = _network(module)
        self.module = module
        self.device = _device_of(w)
        self._buf: Dict[tuple, torch.Tensor] = {}
        self._obs: Optional[torch.Tensor] = None

    def _own(self, k: str, shape, dt=torch.float32) -> torch.Tensor:
        key = (k, tuple(shape))
        if key not in self._buf:
            self._buf = {kk: v for kk, v in self._buf.items() if kk[0] != k}   # one size kept per key
            self._buf[key] = torch.empty(shape, dtype=dt, device=self.device)
        return self._buf[key]

    def _weights(self):
        w, dims = _network(self.module)
        if dims != self.dims or w["w0"].device != self.device:
            raise ValueError("MLPTrainer: the module changed its shape or device")
        return w

    def forward(self, obs: torch.Tensor, *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """logits [rows, 9] of `obs` [rows, in_dim]; `obs` is kept (not copied) for backward()."""
        w = self._weights()
        rows = _check_obs(obs, self.dims, self.device)
        if out is None:
            out = self._own("logits", (rows, NUM_ACTIONS))
        else:
            _check_out(out, (rows, NUM_ACTIONS), torch.float32, self.device)
        h0, h1 = self._own("h0", (rows, self.dims[1])), self._own("h1", (rows, self.dims[2]))
        _run_forward(self.dims, w, obs, h0, h1, out)
        self._obs = obs
        return out

    def activations(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(h0 [rows, hidden0], h1 [rows, hidden1]) of the last forward(): the trainer's own buffers."""
        if self._obs is None:
            raise ValueError("MLPTrainer.activations: no forward() yet")
        rows = self._obs.shape[0]
        return self._own("h0", (rows, self.dims[1])), self._own("h1", (rows, self.dims[2]))

    def backward(self, dlogits: torch.Tensor, out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """The six gradients {"w0" .. "b2"} of sum(logits * dlogits) for the last forward(), in the
        parameters' layouts, overwritten (not accumulated): into `out`'s tensors, or the trainer's own."""
        if self._obs is None:
            raise ValueError("MLPTrainer.backward: no forward() yet")
        w = self._weights()
        obs = self._obs
        rows = obs.shape[0]
        _check_rows(dlogits, "dlogits", NUM_ACTIONS, self.device)
        if dlogits.shape[0] != rows:
            raise ValueError(f"dlogits: expected {rows} rows, got {dlogits.shape[0]}")
        if out is None:
            grads = {k: self._own("g" + k, w[k].shape) for k in KEYS}
        else:
            if sorted(out) != sorted(KEYS):
                raise ValueError(f"out: the six keys {KEYS}, got {sorted(out)}")
            for k in KEYS:
                _check_out(out[k], w[k].shape, torch.float32, self.device)
            grads = dict(out)
        h0, h1 = self._own("h0", (rows, self.dims[1])), self._own("h1", (rows, self.dims[2]))
        work = self._own("work", (work_bytes(self.dims, rows),), torch.uint8)
        _run_backward(self.dims, w, obs, h0, h1, dlogits, grads, work)
        return grads


# ------------------------------------------------------------------ several trainers in one launch per product
def _check_many(trainers, what: str):
    """The list itself: MLPTrainers, at most WH_MLP_TRAIN_MAX_NETS, none twice, one shape, one device."""
    trainers = list(trainers)
    if len(trainers) > nat.WH_MLP_TRAIN_MAX_NETS:
        raise ValueError(f"{what}: at most {nat.WH_MLP_TRAIN_MAX_NETS} trainers in one call, got {len(trainers)}")
    for i, t in enumerate(trainers):
        if not isinstance(t, MLPTrainer):
            raise ValueError(f"{what}: trainers[{i}] is no MLPTrainer")
        if any(t is o for o in trainers[:i]):
            raise ValueError(f"{what}: trainers[{i}] is listed twice (its buffers would be written twice)")
        if t.dims != trainers[0].dims:
            raise ValueError(f"{what}: one network shape per call, got {trainers[0].dims} and {t.dims}")
        if t.device != trainers[0].device:
            raise ValueError(f"{what}: one device per call, got {trainers[0].device} and {t.device}")
    return trainers


def _run_many(name: str, dims, device, jobs, rows: int) -> None:
    arr = (nat.WhMlpTrainJob * len(jobs))(*jobs)
    desc = _desc(dims)
    with torch.cuda.device(device):
        nat.check(getattr(nat.lib(), name)(ctypes.byref(desc), len(jobs), arr, rows, nat.stream_of(device)), name)


def train_forward_many(trainers, obs):
    """`[t.forward(o) for t, o in zip(trainers, obs)]` in three launches for all trainers
    (wh_mlp_train_forward_multi) instead of three each: the same bytes in the same buffers.

    `trainers`: up to four MLPTrainers of one shape on one device, none twice.  `obs`: one [rows, in_dim]
    tensor for all of them, or a list of one per trainer, all of one row count.  Every trainer keeps its
    obs, h0 / h1 and logits as its own forward() does, so `activations()` and a later `backward()` -- its
    own or train_backward_many -- work as after its own forward().  Returns the trainers' logits.  An
    empty list returns an empty list.  ValueError for a bad argument, before any native call."""
    trainers = _check_many(trainers, "train_forward_many")
    if torch.is_tensor(obs):
        obs = [obs] * len(trainers)
    else:
        obs = list(obs)
        if len(obs) != len(trainers):
            raise ValueError(f"train_forward_many: obs is one tensor or one per trainer ({len(trainers)}), got {len(obs)}")
    if not trainers:
        return []
    dims, dev = trainers[0].dims, trainers[0].device
    ws = [t._weights() for t in trainers]
    rows = [_check_obs(o, dims, dev) for o in obs]
    if any(r != rows[0] for r in rows):
        raise ValueError(f"train_forward_many: one row count per call, got {rows}")
    jobs, outs = [], []
    for t, w, o in zip(trainers, ws, obs):
        out = t._own("logits", (rows[0], NUM_ACTIONS))
        h0, h1 = t._own("h0", (rows[0], dims[1])), t._own("h1", (rows[0], dims[2]))
        jobs.append(nat.WhMlpTrainJob(_struct(w), _ptr(o), _ptr(h0), _ptr(h1), _ptr(out), None,
                                      nat.WhMlpGrads(), None))
        outs.append(out)
    if rows[0] > 0:       # (no rows: nothing to launch, and the shared placeholder address is no two buffers)
        _run_many("wh_mlp_train_forward_multi", dims, dev, jobs, rows[0])
    for t, o in zip(trainers, obs):
        t._obs = o
    return outs


def train_backward_many(trainers, dlogits, out=None):
    """`[t.backward(dz, out=o) for ...]` in three launches for all trainers (four above 512 rows;
    wh_mlp_backward_multi): the same bytes in the same buffers.

    `trainers` as for train_forward_many, each after a forward of one row count; `dlogits`: a list of one
    [rows, 9] tensor per trainer; `out`: None, or a list of one dict of six tensors (or None: the
    trainer's own) per trainer.  Returns the list of gradient dicts.  An empty list returns an empty
    list.  ValueError for a bad argument, before any native call."""
    trainers = _check_many(trainers, "train_backward_many")
    if torch.is_tensor(dlogits):
        raise ValueError("train_backward_many: dlogits is a list of one tensor per trainer")
    dlogits = list(dlogits)
    if len(dlogits) != len(trainers):
        raise ValueError(f"train_backward_many: {len(trainers)} dlogits, got {len(dlogits)}")
    outs = [None] * len(trainers) if out is None else list(out)
    if len(outs) != len(trainers):
        raise ValueError(f"train_backward_many: out is None or one entry per trainer ({len(trainers)}), got {len(outs)}")
    if not trainers:
        return []
    dims, dev = trainers[0].dims, trainers[0].device
    for i, t in enumerate(trainers):
        if t._obs is None:
            raise ValueError(f"train_backward_many: trainers[{i}] has had no forward yet")
    rows = [int(t._obs.shape[0]) for t in trainers]
    if any(r != rows[0] for r in rows):
        raise ValueError(f"train_backward_many: one row count per call, the forwards had {rows}")
    rows = rows[0]
    ws = [t._weights() for t in trainers]
    for i, (w, dz, o) in enumerate(zip(ws, dlogits, outs)):       # every check before any native call
        _check_rows(dz, f"dlogits[{i}]", NUM_ACTIONS, dev)
        if dz.shape[0] != rows:
            raise ValueError(f"dlogits[{i}]: expected {rows} rows, got {dz.shape[0]}")
        if o is None:
            continue
        if not isinstance(o, dict) or sorted(o) != sorted(KEYS):
            raise ValueError(f"out[{i}]: None or a dict of the six keys {KEYS}")
        for k in KEYS:
            _check_out(o[k], w[k].shape, torch.float32, dev)
            if any(p is not None and p[k].data_ptr() == o[k].data_ptr() for p in outs[:i]):
                raise ValueError(f"out[{i}][{k!r}]: two trainers' gradients in one tensor")
    jobs, res = [], []
    for t, w, dz, o in zip(trainers, ws, dlogits, outs):
        grads = {k: t._own("g" + k, w[k].shape) for k in KEYS} if o is None else dict(o)
        h0, h1 = t._own("h0", (rows, dims[1])), t._own("h1", (rows, dims[2]))
        work = t._own("work", (work_bytes(dims, rows),), torch.uint8)
        jobs.append(nat.WhMlpTrainJob(_struct(w), _ptr(t._obs), _ptr(h0), _ptr(h1), None, _ptr(dz),
                                      _struct(grads), work.data_ptr()))
        res.append(grads)
    _run_many("wh_mlp_backward_multi", dims, dev, jobs, rows)
    return res
