"""The policy / Q network's training step on the card: warehouse.mlp_logits / MLPTrainer (exact f32
kernels on the module's own parameters, csrc/mlp_train.h) against torch autograd of the same
Sequential, in one process.

    python tools/train_probe.py [--out profiles/mlp_train_probe.txt] [--rounds 5] [--rows 512 4096]

Every variant is warmed up; variants are interleaved per round; device times are HIP events over `reps`
back-to-back calls (median [min .. max] over the rounds).  Per network shape (small / medium / large) and
row count:

  (a)  mlp_logits(module, obs).sum().backward()       the autograd surface: 3 + 3 (4 above 512 rows) launches
                                                       of the kernels, and what autograd adds around them
  (b)  module(obs).sum().backward()                   torch autograd of the same Sequential (the op count
                                                       of forward + backward is printed)
  (c)  MLPTrainer.forward alone                       3 launches
  (d)  MLPTrainer.backward alone                      3 launches (4 above 512 rows)
  (e)  module(obs) under no_grad                      torch's forward alone

(a) and (b) leave their gradients in param.grad (accumulating: the add is part of both).  Before timing,
the gradients of (a) and (b) are compared once.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rllib-warehouse_amd")]

import torch  # noqa: E402
from torch.utils._python_dispatch import TorchDispatchMode  # noqa: E402

import warehouse  # noqa: E402
from warehouse import _native as nat  # noqa: E402
from warehouse.policy import HIDDEN  # noqa: E402
from warehouse._geometry import GEOMETRY  # noqa: E402

LINES = []
DEV = torch.device("cuda", 0)


def say(s):
    print(s, flush=True)
    LINES.append(s)


def time_us(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for r in range(reps):
        fn(r)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps * 1e3


def report(name, samples):
    med = statistics.median(samples)
    say(f"{name:72s} {med:10.2f} us  [{min(samples):.2f} .. {max(samples):.2f}]")
    return med


def run(variants, rounds, reps):
    for _, fn in variants:
        for r in range(3):
            fn(r)
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, fn in variants:
            times[name].append(time_us(fn, reps))
    return {name: report(name, times[name]) for name, _ in variants}


class OpCounter(TorchDispatchMode):
    """Dispatched aten ops that launch a kernel (views and metadata ops left out)."""
    VIEWS = {"view", "reshape", "squeeze", "unsqueeze", "expand", "alias", "detach", "select", "slice", "_unsafe_view",
             "t", "transpose"}

    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if func._schema.name.split("::")[-1] not in self.VIEWS:
            self.n += 1
        return func(*args, **(kwargs or {}))


def probe(variant, rows, rounds, reps):
    in_dim, (h0, h1) = 9 * GEOMETRY[variant]["R"] + 1, HIDDEN[variant]
    torch.manual_seed(1)
    L = torch.nn.Linear
    module = torch.nn.Sequential(L(in_dim, h0), torch.nn.ReLU(), L(h0, h1), torch.nn.ReLU(), L(h1, 9)).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(7)
    obs = torch.rand((rows, in_dim), device=DEV, generator=g) * 2 - 1
    dz = torch.ones((rows, 9), device=DEV)
    trainer = warehouse.MLPTrainer(module)

    def grads():
        return [p.grad.clone() for p in module.parameters()]

    module.zero_grad(set_to_none=True)
    warehouse.mlp_logits(module, obs).sum().backward()
    mine = grads()
    module.zero_grad(set_to_none=True)
    with OpCounter() as oc:
        module(obs).sum().backward()
    theirs = grads()
    rel = max(float((a - b).abs().max() / b.abs().max().clamp(min=1e-30)) for a, b in zip(mine, theirs))

    def a_device(r):
        warehouse.mlp_logits(module, obs).sum().backward()

    def b_torch(r):
        module(obs).sum().backward()

    def c_forward(r):
        trainer.forward(obs)

    def d_backward(r):
        trainer.backward(dz)

    def e_torch_forward(r):
        with torch.no_grad():
            module(obs)

    trainer.forward(obs)
    flop = 3 * 2 * rows * (in_dim * h0 + h0 * h1 + h1 * 9) - 2 * rows * in_dim * h0     # (no gradient w.r.t. obs)
    say(f"## {variant} [{in_dim} -> {h0} -> {h1} -> 9], {rows} rows, {flop / 1e9:.2f} GFLOP forward + backward; "
        f"gradients vs torch autograd: largest |diff| / largest |grad| {rel:.1e}")
    A, B = "(a)  mlp_logits(...).sum().backward()", f"(b)  module(obs).sum().backward(): {oc.n} torch ops"
    C, D, E = "(c)  MLPTrainer.forward", "(d)  MLPTrainer.backward", "(e)  module(obs), no_grad"
    med = run([(A, a_device), (B, b_torch), (C, c_forward), (D, d_backward), (E, e_torch_forward)], rounds, reps)
    say(f"(b) / (a) = {med[B] / med[A]:.2f}   (b) / ((c) + (d)) = {med[B] / (med[C] + med[D]):.2f}   "
        f"(e) / (c) = {med[E] / med[C]:.2f}   (c) + (d): {flop / ((med[C] + med[D]) * 1e-6) / 1e12:.2f} TFLOP/s")
    module.zero_grad(set_to_none=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rows", type=int, nargs="+", default=[512, 4096])
    ap.add_argument("--variants", nargs="+", default=["small", "medium", "large"])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "train_probe measures on the MI355X: no GPU, no numbers"
    say(f"# {nat.lib().wh_version().decode()}  {torch.cuda.get_device_name(0)}")
    for variant in a.variants:
        for rows in a.rows:
            probe(variant, rows, a.rounds, a.reps)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
