"""The forward half of a SAC learner on the device: Q networks, TD targets and TD errors
(include/warehouse_amd.h, SAC TD TARGETS; csrc/sac.h).

The Q_model of scripts/experiments/warehouse-{small,medium,large}-sac/*.yaml has the policy_model's
shape (a ReLU MLP with one output per action), so a Q network is an `MLPPolicy` whose nine outputs
are read as Q values, and it runs on the same kernels from the same operands `ReplayBuffer.sample`
writes.  `SACCritic` holds the policy, the (twin) Q networks and their targets, and turns a sampled
batch into RLlib's discrete-SAC TD target `y`, the per-row TD errors and one TD error per ring entry
-- what `ReplayBuffer.update_priorities` takes -- on the current stream with no host sync:

    critic = SACCritic(policy, q1, q2, q1_target, q2_target, alpha=0.2, gamma=0.99)
    batch = buf.sample(64, fragments=True)
    out = critic.td(batch)                              # y [M,NA], td_rows [M,NA], td [M]
    buf.update_priorities(batch["idx_out"], out["td"])
    policy.load_weights(weights_of(policy_module))      # after the learner's optimiser step
    critic.sync_targets()                               # every target_network_update_freq steps

Soft target updates (tau < 1) are the learner's, in torch; it hands new parameters back with
`MLPPolicy.load_weights`.  A network's own forward under autograd and its backward need not be torch's:
`warehouse.mlp_logits(module, obs)` (warehouse/train.py) is Q(obs) or pi(obs) on the device in exact
f32, read from the module's parameters, and fills `param.grad` on `loss.backward()`.  The losses
(critic, actor, alpha) with their d(loss)/d(logits), the optimiser step, and one `update(batch)` over
all of it are warehouse/learner.py's (`sac_losses`, `DeviceAdam`, `SACLearner`).
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import torch

from . import _native as nat
from .batched import _check_out
from .policy import NUM_ACTIONS, MLPPolicy, forward_many

QNetwork = MLPPolicy   # the same shapes; the 9 outputs are Q(s, a) for the 9 moves

# fused=None takes the one-launch route up to this many agent rows (M x NA): the largest batch at which
# it measured faster.  SACCritic.td on one MI355X, Medium-8, five bf16 networks, fused / sequential in
# us (profiles/mlp_multi_probe.txt): 512 rows 34.7 / 139.0, 4,096 rows 37.5 / 141.9,
# 16,384 rows 67.4 / 146.0, 32,768 rows 95.4 / 149.7, 49,152 rows 124.6 / 156.3 -- and then the five
# networks' 1,280 tasks share the launch's 256 workgroups where a launch each has 256 of its own:
# 65,536 rows 174.9 / 166.4, 262,144 rows 613.7 / 602.6.  Above the threshold auto runs sequentially.
FUSED_MAX_ROWS = 49152


class SACCritic:
    def __init__(self, policy: MLPPolicy, q1: MLPPolicy, q2: Optional[MLPPolicy], q1_target: MLPPolicy,
                 q2_target: Optional[MLPPolicy], *, alpha: float, gamma: float = 0.99, n_step: int = 1,
                 mask_dones: bool = False, fused: Optional[bool] = None):
        """`q2` and `q2_target` may both be None (no twin Q).  `alpha` (the entropy coefficient) is
        a plain attribute: a learner sets it from its log_alpha before a call.  `mask_dones=False`
        is what the YAMLs train with (no_done_at_end: true): the bootstrap ignores the done flag.
        `fused`: True issues a call's three or five forwards as ONE launch (policy.forward_many) and
        needs every network to have one shape and precision; False runs them one after the other;
        None (default) takes the one launch when the networks allow it and the batch has at most
        FUSED_MAX_ROWS agent rows.  Both routes give the same bits.  `last_fused` says which route
        the last call took."""
        if (q2 is None) != (q2_target is None):
            raise ValueError("SACCritic: q2 and q2_target come together (both, or neither)")
        nets = [n for n in (policy, q1, q2, q1_target, q2_target) if n is not None]
        for n in nets:
            if not isinstance(n, MLPPolicy):
                raise ValueError("SACCritic: the networks are MLPPolicy / QNetwork objects")
            if (n.in_dim, n.device) != (policy.in_dim, policy.device):
                raise ValueError("SACCritic: every network takes the policy's rows, on the policy's device")
        self.policy, self.q1, self.q2, self.q1_target, self.q2_target = policy, q1, q2, q1_target, q2_target
        self.device = policy.device
        self.alpha = float(alpha)
        self.gamma = float(gamma)
        self.n_step = int(n_step)
        self.mask_dones = bool(mask_dones)
        self._buf: Dict[tuple, torch.Tensor] = {}
        self.one_shape = all((n.hidden, n.precision) == (policy.hidden, policy.precision) for n in nets)
        if fused and not self.one_shape:
            raise ValueError("SACCritic: fused=True needs every network to have one shape and precision")
        self.fused = None if fused is None else bool(fused)
        self.last_fused: Optional[bool] = None

    def use_fused(self, rows: int) -> bool:
        """Whether a call over `rows` agent rows takes the one-launch route."""
        if self.fused is None:
            return self.one_shape and rows <= FUSED_MAX_ROWS
        return self.fused

    # ------------------------------------------------------------------ buffers
    def _own(self, k: str, shape, dt=torch.float32) -> torch.Tensor:
        key = (k, tuple(shape))
        if key not in self._buf:
            self._buf = {kk: v for kk, v in self._buf.items() if kk[0] != k}   # one size kept per key
            self._buf[key] = torch.empty(shape, dtype=dt, device=self.device)
        return self._buf[key]

    def _forward(self, net: MLPPolicy, batch, side: str, rows: int, name: str) -> torch.Tensor:
        """The logits of `net` on one side of the batch ("" = obs, "next_" = next_obs), into a
        critic-owned [rows, 9] buffer: from the fragment operand when the batch has it and the
        network is bf16, else from the f32 rows."""
        out = self._own(name, (rows, NUM_ACTIONS))
        scratch = self._own("actions", (rows,), torch.int32)
        frag, obs = batch.get(side + "xfrag"), batch.get(side + "obs")
        if frag is not None and net.precision == "bf16":
            net.forward_x(frag, rows, logits=out, actions=scratch, step=0)
        elif obs is not None:
            net.forward(obs.view(rows, -1), logits=out, actions=scratch, step=0)
        else:
            raise ValueError(f"SACCritic: the batch holds no {side}obs rows" +
                             (" (an f32 network reads rows: sample(rows=True))" if frag is not None else
                              f" and no {side}xfrag operand"))
        return out

    def _forward_fused(self, batch, rows: int, with_q: bool):
        """_forward for all of a call's networks in one launch: logits only, so no action is computed
        (NULL goes to the ABI) and no scratch buffer is touched."""
        plan = [(self.policy, "next_", "pi_next"), (self.q1_target, "next_", "q1t_next"),
                (self.q2_target, "next_", "q2t_next"), (self.q1 if with_q else None, "", "q1"),
                (self.q2 if with_q else None, "", "q2")]
        jobs, outs = [], []
        for net, side, name in plan:
            if net is None:
                outs.append(None)
                continue
            out = self._own(name, (rows, NUM_ACTIONS))
            frag, obs = batch.get(side + "xfrag"), batch.get(side + "obs")
            if frag is not None and net.precision == "bf16":
                jobs.append(dict(net=net, xfrag=frag, rows=rows, logits=out, step=0))
            elif obs is not None:
                jobs.append(dict(net=net, obs=obs.view(rows, -1), logits=out, step=0))
            else:
                raise ValueError(f"SACCritic: the batch holds no {side}obs rows" +
                                 (" (an f32 network reads rows: sample(rows=True))" if frag is not None else
                                  f" and no {side}xfrag operand"))
            outs.append(out)
        forward_many(jobs)
        return outs

    def _run(self, batch, out, with_q: bool, log_alpha=None) -> Dict[str, torch.Tensor]:
        if log_alpha is not None and (not torch.is_tensor(log_alpha) or log_alpha.numel() != 1 or
                                      log_alpha.dtype != torch.float32 or log_alpha.device != self.device):
            raise ValueError(f"SACCritic: log_alpha is a one-element float32 tensor on {self.device}")
        for k in ("actions", "rewards"):
            if k not in batch:
                raise ValueError(f"SACCritic: the batch lacks {k!r}")
        M, NA = batch["rewards"].shape
        rows = M * NA
        keys = ("y", "td_rows", "td") if with_q else ("y",)
        shapes = dict(y=(M, NA), td_rows=(M, NA), td=(M,))
        if out is None:
            res = {k: self._own("out_" + k, shapes[k]) for k in keys}
        else:
            res = dict(out)
            if not res or any(k not in keys for k in res):
                raise ValueError(f"out: some of {keys}, got {sorted(res)}")
            for k, v in res.items():
                _check_out(v, shapes[k], torch.float32, self.device)
        if self.mask_dones and "dones" not in batch:
            raise ValueError("SACCritic: mask_dones needs the batch's dones")
        if M == 0:
            return res
        self.last_fused = self.use_fused(rows)
        if self.last_fused:
            pi, q1t, q2t, q1, q2 = self._forward_fused(batch, rows, with_q)
            return self._epilogue(batch, res, M, NA, pi, q1t, q2t, q1, q2, log_alpha)
        pi = self._forward(self.policy, batch, "next_", rows, "pi_next")
        q1t = self._forward(self.q1_target, batch, "next_", rows, "q1t_next")
        q2t = self._forward(self.q2_target, batch, "next_", rows, "q2t_next") if self.q2_target is not None else None
        q1 = self._forward(self.q1, batch, "", rows, "q1") if with_q else None
        q2 = self._forward(self.q2, batch, "", rows, "q2") if with_q and self.q2 is not None else None
        return self._epilogue(batch, res, M, NA, pi, q1t, q2t, q1, q2, log_alpha)

    def _epilogue(self, batch, res, M, NA, pi, q1t, q2t, q1, q2, log_alpha=None):
        n, dones = batch.get("n"), batch.get("dones")
        args = nat.WhSacTdArgs(pi.data_ptr(), q1t.data_ptr(), nat.ptr(q2t), nat.ptr(q1), nat.ptr(q2),
                               nat.ptr(batch["actions"]), nat.ptr(batch["rewards"]), nat.ptr(dones), nat.ptr(n),
                               self.alpha, self.gamma ** self.n_step, int(self.mask_dones),
                               nat.ptr(res.get("y")), nat.ptr(res.get("td_rows")), nat.ptr(res.get("td")))
        if log_alpha is not None:   # alpha = exp(log_alpha[0]) on the device; args.alpha is ignored
            nat.check(nat.lib().wh_sac_td_la(M, NA, ctypes.byref(args), log_alpha.data_ptr(),
                                             nat.stream_of(self.device)), "wh_sac_td_la")
            return res
        nat.check(nat.lib().wh_sac_td(M, NA, ctypes.byref(args), nat.stream_of(self.device)), "wh_sac_td")
        return res

    # ------------------------------------------------------------------ the surface
    def td(self, batch: Dict[str, torch.Tensor], *, out: Optional[Dict[str, torch.Tensor]] = None,
           log_alpha: Optional[torch.Tensor] = None):
        """`batch`: a ReplayBuffer.sample(..., fragments=True) dict (bf16 networks read the xfrag /
        next_xfrag operands), or one with rows (obs / next_obs; what f32-precision networks read).
        Runs the policy and the target Q networks on the next side and the Q networks on the obs
        side (five forwards, three without a twin), then wh_sac_td.  Returns {"y" [M,NA], "td_rows"
        [M,NA], "td" [M]}: the critic's own tensors, overwritten by its next call, or the caller's
        through `out` (any of the three keys).  td[m] is one TD error per ring entry, the mean over
        its live agent rows: `buf.update_priorities(batch["idx_out"], out["td"])`.  `log_alpha`: None
        uses `self.alpha`; a one-element float32 tensor on the critic's device makes the kernel read it
        and use alpha = exp(log_alpha) (wh_sac_td_la): no host read, and the value a replayed stream
        capture sees is the one in memory then."""
        return self._run(batch, out, True, log_alpha)

    def targets(self, batch: Dict[str, torch.Tensor], *, out: Optional[Dict[str, torch.Tensor]] = None,
                log_alpha: Optional[torch.Tensor] = None):
        """Only the three next-side forwards and {"y"}: for a learner that wants the target without
        gradient and computes Q(obs) itself under autograd.  The same `y` as td(), bit for bit
        (`log_alpha` as in td())."""
        return self._run(batch, out, False, log_alpha)

    def sync_targets(self) -> None:
        """q1_target <- q1 and q2_target <- q2 (MLPPolicy.copy_from): the YAMLs' hard target update."""
        self.q1_target.copy_from(self.q1)
        if self.q2_target is not None:
            self.q2_target.copy_from(self.q2)
