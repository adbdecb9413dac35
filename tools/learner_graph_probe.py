"""SACLearner.update three ways in one process: the default route (one host read per update), the
sync-free route (sync_free=True: alpha and Adam's step count read on the device), and a replay of the
captured sync-free update (SACLearner.capture).

    python tools/learner_graph_probe.py [--out profiles/learner_graph_probe.txt] [--rounds 5] [--reps 20]

The protocol of tools/train_multi_probe.py: every route is warmed up; routes are
interleaved per round; times are HIP events around `reps` back-to-back calls (median [min .. max] over the
rounds), and beside each span the host's own time to enqueue the same calls (perf_counter around the loop,
before any synchronisation): where the two are equal the device waits for the host.  Small-4 and Medium-8
at M = 64 (the YAMLs' train_batch_size) and M = 512, five bf16 critic networks, a uniform ring (no
priorities: the three routes time the update alone).  The default route is the baseline: the code of the
parent tree, in the same process.
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
CONFIGS = (("small", 4), ("medium", 8))


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


def module(variant, seed):
    in_dim, (h0, h1) = 9 * GEOMETRY[variant]["R"] + 1, HIDDEN[variant]
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(in_dim, h0), torch.nn.ReLU(), torch.nn.Linear(h0, h1), torch.nn.ReLU(),
                               torch.nn.Linear(h1, 9)).to(DEV)


def learner(variant, sync_free):
    mods = [module(variant, 20 + i) for i in range(3)]
    nets = [MLPPolicy(variant, seed=20 + i) for i in range(5)]
    for net, m in zip(nets[:3], mods):
        net.load_weights(weights_of(m))
    critic = warehouse.SACCritic(nets[0], nets[1], nets[2], nets[3], nets[4], alpha=1.0, gamma=0.99)
    return warehouse.SACLearner(*mods, rollout_policy=nets[0], critic=critic, log_alpha=torch.zeros(1, device=DEV),
                                sync_free=sync_free)


def leg(variant, na, M, rounds, reps):
    env = warehouse.BatchedWarehouse(variant, 64, na, seed=3, device=DEV)
    env.reset()
    buf = warehouse.ReplayBuffer(env, capacity=16)
    for _ in range(16):
        buf.step(env.policy("greedy", 0.2))
    batch = {k: v.clone() for k, v in buf.sample(M, rows=True, fragments=True).items()}
    eager, free, held = learner(variant, False), learner(variant, True), learner(variant, True)
    graph = held.capture(batch)
    routes = [("update(), sync_free=False (the default)", lambda: eager.update(batch)),
              ("update(), sync_free=True", lambda: free.update(batch)),
              ("capture(batch).replay()", graph.replay)]
    for _, fn in routes:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    dev = {name: [] for name, _ in routes}
    host = {name: [] for name, _ in routes}
    for _ in range(rounds):
        for name, fn in routes:
            d, h = time_us(fn, reps)
            dev[name].append(d)
            host[name].append(h)
    say(f"{variant.capitalize()}-{na}, M = {M} ({M * na} rows): one whole learner update, five bf16 critic networks")
    for name, _ in routes:
        v, h = dev[name], host[name]
        say(f"    {name:<42s} {statistics.median(v):8.1f} us  [{min(v):.1f} .. {max(v):.1f}]   host enqueue "
            f"{statistics.median(h):7.1f} us  [{min(h):.1f} .. {max(h):.1f}]")
    base = dev[routes[0][0]]
    spread = max(base) - min(base)
    for name, _ in routes[1:]:
        gain = statistics.median(base) - statistics.median(dev[name])
        say(f"    {name} is {gain:+.1f} us faster than the default at the medians; the default's rounds spread over "
            f"{spread:.1f} us: {'a win beyond the spread' if gain > spread else 'no win beyond the spread'}")
    torch.cuda.synchronize()
    same = all(torch.equal(x, y) for x, y in zip(free.params, held.params)) and free.updates == held.updates
    say(f"    after {free.updates} updates each the eager sync-free and the replayed learner's parameters are "
        f"{'bit-equal' if same else 'DIFFERENT'} (Adam's clock: t = {free.adam.t} and {held.adam.t})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "learner_graph_probe.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("learner_graph_probe: no HIP device: the probe measures on the MI355X and has no fallback")
    sha = nat.verify_provenance()
    say(f"# python tools/learner_graph_probe.py --rounds {a.rounds} --reps {a.reps}   ({torch.cuda.get_device_name(0)}, "
        f"library sha {sha})")
    say(f"# HIP events around {a.reps} back-to-back calls, us per call: median [min .. max] over {a.rounds} interleaved "
        "rounds; beside it the host's time to enqueue the same calls")
    for variant, na in CONFIGS:
        for M in (64, 512):
            leg(variant, na, M, a.rounds, a.reps)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
