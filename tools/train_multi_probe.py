"""A learner's three training passes one network after the other against all three in one launch per
product (train_forward_many / train_backward_many, SACLearner(fused_train=True)), in one process.

    python tools/train_multi_probe.py [--out profiles/mlp_train_multi_probe.txt] [--rounds 5] [--reps 20]

The protocol of tools/mlp_multi_probe.py and tools/learner_probe.py: every variant is warmed up; variants
are interleaved per round; times are HIP events around `reps` back-to-back calls (median [min .. max]
over the rounds).  At these launch-bound sizes a span is partly host time, so the host's own time to
enqueue the same calls (perf_counter around the loop, before any synchronisation) is printed beside it:
where the two are equal the device waits for the host.  Medium-8 and Small-4 at M = 64 (the YAMLs'
train_batch_size) and M = 512.

  (a) three MLPTrainer.forward calls against one train_forward_many
  (b) three MLPTrainer.backward calls against one train_backward_many
  (c) SACLearner.update with fused_train=False against fused_train=True

The sequential route is the baseline: the same code in the same process.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rllib-warehouse_amd")]

import torch  # noqa: E402

import warehouse  # noqa: E402
from warehouse import _native as nat  # noqa: E402
from warehouse.policy import HIDDEN, MLPPolicy, weights_of  # noqa: E402
from warehouse._geometry import GEOMETRY  # noqa: E402

LINES = []
DEV = torch.device("cuda", 0)
CONFIGS = (("medium", 8), ("small", 4))


def say(s):
    print(s, flush=True)
    LINES.append(s)


def time_us(fn, reps):
    """(HIP-event span, host enqueue time), us per call."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    h0 = time.perf_counter()
    for _ in range(reps):
        fn()
    h1 = time.perf_counter()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1000.0 / reps, (h1 - h0) * 1e6 / reps


def compare(title, variants, rounds, reps):
    for _, fn in variants:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    dev = {name: [] for name, _ in variants}
    host = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, fn in variants:
            d, h = time_us(fn, reps)
            dev[name].append(d)
            host[name].append(h)
    say(title)
    for name, _ in variants:
        v, h = dev[name], host[name]
        say(f"    {name:<46s} {statistics.median(v):8.1f} us  [{min(v):.1f} .. {max(v):.1f}]   host enqueue "
            f"{statistics.median(h):7.1f} us  [{min(h):.1f} .. {max(h):.1f}]")
    return dev


def module(variant, seed):
    in_dim, (h0, h1) = 9 * GEOMETRY[variant]["R"] + 1, HIDDEN[variant]
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(in_dim, h0), torch.nn.ReLU(), torch.nn.Linear(h0, h1), torch.nn.ReLU(),
                               torch.nn.Linear(h1, 9)).to(DEV)


def section_passes(variant, na, M, rounds, reps):
    rows = M * na
    mods = [module(variant, 30 + i) for i in range(3)]
    g = torch.Generator(device="cpu").manual_seed(rows)
    obs = (torch.rand(rows, mods[0][0].in_features, generator=g) * 2 - 1).to(DEV)
    dz = [((torch.rand(rows, 9, generator=g) * 2 - 1) / rows).to(DEV) for _ in range(3)]
    seq = [warehouse.MLPTrainer(m) for m in mods]
    many = [warehouse.MLPTrainer(m) for m in mods]
    a = [t.forward(obs).clone() for t in seq]
    b = warehouse.train_forward_many(many, obs)
    ga = [{k: v.clone() for k, v in t.backward(d).items()} for t, d in zip(seq, dz)]
    gb = warehouse.train_backward_many(many, dz)
    same = all(torch.equal(x, y) for x, y in zip(a, b)) and all(torch.equal(x[k], y[k]) for x, y in zip(ga, gb) for k in x)
    head = f"{variant.capitalize()}-{na}, M = {M} ({rows} rows)"
    say(f"{head}: the two routes' logits and gradients are {'bit-equal' if same else 'DIFFERENT'}")
    compare(f"(a) {head}: three training forwards",
            [("3 x MLPTrainer.forward (9 launches)", lambda: [t.forward(obs) for t in seq]),
             ("train_forward_many (3 launches)", lambda: warehouse.train_forward_many(many, obs))], rounds, reps)
    nb = 3 if rows <= 512 else 4
    compare(f"(b) {head}: three backwards",
            [(f"3 x MLPTrainer.backward ({3 * nb} launches)", lambda: [t.backward(d) for t, d in zip(seq, dz)]),
             (f"train_backward_many ({nb} launches)", lambda: warehouse.train_backward_many(many, dz))], rounds, reps)


def section_update(variant, na, M, rounds, reps):
    env = warehouse.BatchedWarehouse(variant, 64, na, seed=3, device=DEV)
    env.reset()
    buf = warehouse.ReplayBuffer(env, capacity=16)
    for _ in range(16):
        buf.step(env.policy("greedy", 0.2))
    batch = {k: v.clone() for k, v in buf.sample(M, rows=True, fragments=True).items()}

    def learner(fused_train):
        mods = [module(variant, 20 + i) for i in range(3)]
        nets = [MLPPolicy(variant, seed=20 + i) for i in range(5)]
        for net, m in zip(nets[:3], mods):
            net.load_weights(weights_of(m))
        critic = warehouse.SACCritic(nets[0], nets[1], nets[2], nets[3], nets[4], alpha=1.0, gamma=0.99)
        return warehouse.SACLearner(*mods, rollout_policy=nets[0], critic=critic, log_alpha=torch.zeros(1, device=DEV),
                                    fused_train=fused_train)

    seq, fused = learner(False), learner(True)
    got = compare(f"(c) {variant.capitalize()}-{na}, M = {M} ({M * na} rows): one whole SACLearner.update, five bf16 critic networks",
                  [("SACLearner(fused_train=False).update", lambda: seq.update(batch)),
                   ("SACLearner(fused_train=True).update", lambda: fused.update(batch))], rounds, reps)
    s, f = got["SACLearner(fused_train=False).update"], got["SACLearner(fused_train=True).update"]
    gain, spread = statistics.median(s) - statistics.median(f), max(s) - min(s)
    say(f"    fused is {gain:+.1f} us faster at the medians; the sequential route's rounds spread over {spread:.1f} us: "
        f"{'a win beyond the spread' if gain > spread else 'no win beyond the spread'}")
    same = all(torch.equal(x, y) for x, y in zip(seq.params, fused.params))
    say(f"    after {3 + rounds * reps} updates each the two learners' parameters are {'bit-equal' if same else 'DIFFERENT'}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp_train_multi_probe.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("train_multi_probe: no HIP device: the probe measures on the MI355X and has no fallback")
    sha = nat.verify_provenance()
    say(f"# python tools/train_multi_probe.py --rounds {a.rounds} --reps {a.reps}   ({torch.cuda.get_device_name(0)}, "
        f"library sha {sha})")
    say(f"# HIP events around {a.reps} back-to-back calls, us per call: median [min .. max] over {a.rounds} interleaved "
        "rounds; beside it the host's time to enqueue the same calls")
    for variant, na in CONFIGS:
        for M in (64, 512):
            section_passes(variant, na, M, a.rounds, a.reps)
    for variant, na in CONFIGS:
        for M in (64, 512):
            section_update(variant, na, M, a.rounds, a.reps)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
