"""A SAC learner update on the card against the torch routes it replaces, in one process.

    python tools/learner_probe.py [--out profiles/learner_probe.txt] [--rounds 5] [--reps 20]

Every variant is warmed up; variants are interleaved per round; times are HIP events around `reps`
back-to-back calls (median [min .. max] over the rounds), so at these launch-bound sizes they are partly
host times: the span includes whatever the host takes to enqueue the calls.  Medium-8, M = 64 (the YAMLs'
train_batch_size) and M = 512.

  (a) warehouse.sac_losses (wh_sac_loss) against the same formulas as torch ops on the same logits (the
      op count is printed)
  (b) one DeviceAdam.step (wh_adam_step) over the learner's 19 tensors against four torch.optim.Adam
      instances (policy, q1, q2, log_alpha), in torch's default and fused=True forms
  (c) SACLearner.update against the same update written with SACCritic.td + mlp_logits + torch losses +
      four torch.optim.Adam + load_weights: the best route before this one
"""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rllib-warehouse_amd")]

import torch  # noqa: E402
from torch.utils._python_dispatch import TorchDispatchMode  # noqa: E402

import warehouse  # noqa: E402
from warehouse import _native as nat  # noqa: E402
from warehouse.policy import MLPPolicy, weights_of  # noqa: E402

LINES = []
DEV = torch.device("cuda", 0)
NA, TE = 8, 0.935
DIMS = (82, 512, 512)


def say(s):
    print(s, flush=True)
    LINES.append(s)


def time_us(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1000.0 / reps


def compare(title, variants, rounds, reps):
    """variants: [(name, fn)]; warm-up, then `rounds` interleaved rounds."""
    for _, fn in variants:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    got = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, fn in variants:
            got[name].append(time_us(fn, reps))
    say(title)
    for name, _ in variants:
        v = got[name]
        say(f"    {name:<58s} {statistics.median(v):9.1f} us  [{min(v):.1f} .. {max(v):.1f}]")
    return {k: statistics.median(v) for k, v in got.items()}


class OpCount(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.n += 1
        return func(*args, **(kwargs or {}))


def module(seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(DIMS[0], DIMS[1]), torch.nn.ReLU(), torch.nn.Linear(DIMS[1], DIMS[2]),
                               torch.nn.ReLU(), torch.nn.Linear(DIMS[2], 9)).to(DEV)


def torch_losses(pi, q1, q2, y, actions, n, weights, log_alpha, scale):
    """The formulas of wh_sac_loss as torch ops: (actor, critic 1, critic 2, alpha loss), each a scalar
    whose backward gives the gradients; pi / q1 / q2 may require grad."""
    M, na = y.shape
    live = (torch.arange(na, device=y.device)[None, :] < n.clamp(0, na)[:, None]).reshape(-1).to(pi.dtype)
    a = actions.reshape(-1).long()
    a = torch.where((a >= 0) & (a < 9), a, torch.full_like(a, 4))
    w = (weights if weights is not None else torch.ones(M, device=y.device)).repeat_interleave(na)
    logp = torch.log_softmax(pi, dim=1)
    p = logp.exp()
    alpha = log_alpha.detach().exp()
    qm = torch.minimum(q1, q2).detach()
    actor = scale * ((p * (alpha * logp - qm)).sum(dim=1) * live).sum()
    yy = y.reshape(-1)
    e1 = q1.gather(1, a[:, None])[:, 0] - yy
    e2 = q2.gather(1, a[:, None])[:, 0] - yy
    c1 = scale * (0.5 * w * e1 * e1 * live).sum()
    c2 = scale * (0.5 * w * e2 * e2 * live).sum()
    alpha_loss = -log_alpha[0] * scale * ((p.detach() * (logp.detach() + TE)).sum(dim=1) * live).sum()
    return actor, c1, c2, alpha_loss


def section_losses(M, rounds, reps):
    rows = M * NA
    g = torch.Generator(device="cpu").manual_seed(M)
    pi = (torch.rand(rows, 9, generator=g) * 8 - 4).to(DEV)
    q1, q2 = ((torch.rand(rows, 9, generator=g) * 20 - 10).to(DEV) for _ in range(2))
    y = (torch.rand(M, NA, generator=g) * 40 - 20).to(DEV)
    actions = torch.randint(0, 9, (M, NA), generator=g, dtype=torch.int32).to(DEV)
    n = torch.full((M,), NA, dtype=torch.int32, device=DEV)
    weights = (torch.rand(M, generator=g) * 0.75 + 0.25).to(DEV)
    log_alpha = torch.full((1,), math.log(0.2), device=DEV)
    scale = 1.0 / rows

    def device():
        warehouse.sac_losses(pi, q1, q2, y, actions, log_alpha=log_alpha, target_entropy=TE, n=n, weights=weights)

    leaves = [t.clone().requires_grad_() for t in (pi, q1, q2)]
    la = log_alpha.clone().requires_grad_()

    def torch_route():
        for t in leaves + [la]:
            t.grad = None
        actor, c1, c2, al = torch_losses(*leaves, y, actions, n, weights, la, scale)
        (actor + c1 + c2 + al).backward()

    torch_route()
    with OpCount() as oc:
        torch_route()
    got = warehouse.sac_losses(pi, q1, q2, y, actions, log_alpha=log_alpha, target_entropy=TE, n=n, weights=weights)
    err = max(float((got[k] - t.grad).abs().max()) for k, t in zip(("dpi", "dq1", "dq2"), leaves))
    res = compare(f"(a) losses and d(loss)/d(logits), M = {M} ({rows} rows); largest |device - torch| gradient {err:.2e}",
                  [("warehouse.sac_losses: wh_sac_loss" + (", 2 launches" if M * NA > 256 else ", 1 launch"), device),
                   (f"torch ops + autograd on the same logits ({oc.n} dispatched ops)", torch_route)], rounds, reps)
    return res


def learner_tensors(seed):
    mods = [module(seed + i) for i in range(3)]
    return mods, [weights_of(m)[k] for m in mods for k in ("w0", "b0", "w1", "b1", "w2", "b2")]


def section_adam(rounds, reps):
    mods, params = learner_tensors(10)
    log_alpha = torch.zeros(1, device=DEV)
    tensors = params + [log_alpha]
    grads = [torch.randn_like(t) for t in tensors]
    dev = warehouse.DeviceAdam(tensors)

    def torch_opts(**kw):
        ms, _ = learner_tensors(10)
        la = torch.zeros(1, device=DEV, requires_grad=True)
        groups = [list(m.parameters()) for m in ms] + [[la]]
        opts = [torch.optim.Adam(g, lr=3e-4, **kw) for g in groups]
        for p, g in zip([p for grp in groups for p in grp], grads):
            p.grad = g.clone()

        def step():
            for o in opts:
                o.step()
        return step

    default, fused = torch_opts(), torch_opts(fused=True)
    elems = sum(t.numel() for t in tensors)
    return compare(f"(b) one Adam step over the learner's {len(tensors)} tensors ({elems:,} elements, {28 * elems / 1e6:.1f} MB moved)",
                   [("DeviceAdam.step: wh_adam_step, 1 launch", lambda: dev.step(grads)),
                    ("four torch.optim.Adam, default (foreach)", default),
                    ("four torch.optim.Adam, fused=True", fused)], rounds, reps)


def section_update(M, rounds, reps):
    env = warehouse.BatchedWarehouse("medium", 64, NA, seed=3, device=DEV)
    env.reset()
    buf = warehouse.ReplayBuffer(env, capacity=16)
    for _ in range(16):
        buf.step(env.policy("greedy", 0.2))
    batch = {k: v.clone() for k, v in buf.sample(M, rows=True, fragments=True).items()}
    obs = batch["obs"].view(M * NA, -1)
    scale = 1.0 / (M * NA)

    def parts(seed):
        mods = [module(seed + i) for i in range(3)]
        nets = [MLPPolicy("medium", seed=seed + i) for i in range(5)]
        for net, m in zip(nets[:3], mods):
            net.load_weights(weights_of(m))
        critic = warehouse.SACCritic(nets[0], nets[1], nets[2], nets[3], nets[4], alpha=1.0, gamma=0.99)
        return mods, nets, critic

    mods, nets, critic = parts(20)
    learner = warehouse.SACLearner(*mods, rollout_policy=nets[0], critic=critic, log_alpha=torch.zeros(1, device=DEV))

    tm, tn, tc = parts(20)
    la = torch.zeros(1, device=DEV, requires_grad=True)
    opts = [torch.optim.Adam(m.parameters(), lr=3e-4) for m in tm] + [torch.optim.Adam([la], lr=3e-4)]

    def torch_update():
        tc.alpha = math.exp(float(la.item()))
        td = tc.td(batch)
        logits = [warehouse.mlp_logits(m, obs) for m in tm]
        for o in opts:
            o.zero_grad(set_to_none=True)
        actor, c1, c2, al = torch_losses(*logits, td["y"], batch["actions"], batch["n"], None, la, scale)
        (actor + c1 + c2 + al).backward()
        for o in opts:
            o.step()
        for net, m in zip(tn[:3], tm):
            net.load_weights(weights_of(m))

    return compare(f"(c) one whole learner update, M = {M} ({M * NA} rows), five bf16 critic networks on fragments",
                   [("SACLearner.update", lambda: learner.update(batch)),
                    ("SACCritic.td + mlp_logits + torch losses + 4 torch Adam + repack", torch_update)], rounds, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "learner_probe.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("learner_probe: no HIP device: the probe measures on the MI355X and has no fallback")
    sha = nat.verify_provenance()
    say(f"# python tools/learner_probe.py --rounds {a.rounds} --reps {a.reps}   ({torch.cuda.get_device_name(0)}, "
        f"library sha {sha})")
    say(f"# HIP events around {a.reps} back-to-back calls, us per call: median [min .. max] over {a.rounds} interleaved "
        "rounds; partly host times (launch-bound sizes)")
    for M in (64, 512):
        section_losses(M, a.rounds, a.reps)
    section_adam(a.rounds, a.reps)
    for M in (64, 512):
        section_update(M, a.rounds, a.reps)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
