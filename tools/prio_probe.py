"""Prioritized replay sampling through the priority tree against the torch route it replaces, on the
card, in one process.

    python tools/prio_probe.py [--out profiles/prio_probe.txt] [--rounds 5]

Medium-8, B = 65,536; capacity 16 (1.05 M leaves) and capacity 200 (13.1 M leaves); M = 64 (the
reference YAMLs' train_batch_size) and M = 32,768.  Variants, every one warmed up, interleaved per
round and timed with HIP events (median [min .. max] over the rounds):

  sample + gather
    (a)  wh_replay_prio_sample + wh_replay_gather(idx): the two launches
    (a') ReplayBuffer.sample(M) of a prioritized buffer: (a) plus the importance weights in torch
    (b)  the torch route: an f32 priority vector of capacity * B entries, cumsum, searchsorted of M
         uniform draws, then ReplayBuffer.sample(M, idx=...)
    (b') (b) plus the weights (a') computes, by the same torch expression on the gathered priorities
  update of M priorities (both given the same (|td| + eps) ** alpha, computed before the clock starts)
    (a)  wh_replay_prio_update (its two launches)
    (b)  index_put_ on the f32 vector
  recording
    ReplayBuffer.step with and without prioritized=True (the fill's cost per recorded step)
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rllib-warehouse_amd")]

import torch  # noqa: E402

import warehouse  # noqa: E402
from warehouse import _native as nat  # noqa: E402

LINES = []


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
    say(f"{name:64s} {med:9.2f} us  [{min(samples):.2f} .. {max(samples):.2f}]")
    return med


def run(variants, rounds, reps):
    for _, fn in variants:
        for r in range(4):
            fn(r)
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, fn in variants:
            times[name].append(time_us(fn, reps))
    return {name: report(name, times[name]) for name, _ in variants}


def probe(variant, na, B, cap, Ms, rounds, reps, steps=True):
    dev = torch.device("cuda", 0)
    env = warehouse.BatchedWarehouse(variant, B, na, seed=3, device=dev)
    env.reset()
    env.stagger(torch.arange(B, device=dev) % 7)
    buf = warehouse.ReplayBuffer(env, cap, prioritized=True)
    for s in range(cap):
        buf.step(env.policy("greedy", 0.1), observe=False)
    N = len(buf)
    g = torch.Generator(device=dev).manual_seed(5)
    # spread priorities: a sixteenth of the entries updated once
    ix0 = torch.randint(0, N, (N // 16,), device=dev, generator=g)
    buf.update_priorities(ix0, torch.randn(N // 16, device=dev, generator=g) * 3.0)
    vec = (buf.prio_leaf[:N].to(torch.float32) / float(nat.WH_PRIO_ONE)).contiguous()   # route (b)'s priorities
    torch.cuda.synchronize()
    tree_mb = (buf.prio_leaf.numel() * 4 + buf.prio_node.numel() * 8) / 1e6
    say(f"# {variant}-{na}  B = {B}  capacity = {cap}  leaves = {N}  levels = {buf.prio_levels}  "
        f"tree {tree_mb:.1f} MB  f32 vector {vec.numel() * 4 / 1e6:.1f} MB")
    tp, lib = ctypes.byref(buf._tree), env._lib
    for M in Ms:
        shapes = buf._shapes(M)
        keys = ("obs", "next_obs", "actions", "rewards", "dones", "n", "idx_out")
        outs = [{k: torch.empty(shapes[k][0], dtype=shapes[k][1], device=dev) for k in keys} for _ in range(2)]
        tix = torch.empty(M, dtype=torch.int64, device=dev)
        tq = torch.empty(M, dtype=torch.int32, device=dev)
        tot = torch.empty(1, dtype=torch.int64, device=dev)

        def a_kernels(r):
            rc = lib.wh_replay_prio_sample(tp, M, None, env.seed, r, tix.data_ptr(), tq.data_ptr(), tot.data_ptr(),
                                           env.stream)
            assert rc == 0
            buf.sample(M, idx=tix, out=outs[r % 2])

        def a_buffer(r):
            buf.sample(M, draw=r, out=outs[r % 2])

        def b_torch(r):
            c = torch.cumsum(vec, 0)
            u = torch.rand(M, device=dev) * c[-1]
            ix = torch.searchsorted(c, u).clamp_(max=N - 1)
            buf.sample(M, idx=ix, out=outs[r % 2])

        def b_torch_weights(r):
            c = torch.cumsum(vec, 0)
            u = torch.rand(M, device=dev) * c[-1]
            ix = torch.searchsorted(c, u).clamp_(max=N - 1)
            pq = vec[ix].to(torch.float64)
            ((pq / pq.min()) ** -0.4).to(torch.float32)
            buf.sample(M, idx=ix, out=outs[r % 2])

        uix = torch.randint(0, N, (M,), device=dev, generator=g)
        p = ((torch.randn(M, device=dev, generator=g) * 3.0).abs() + buf.eps) ** buf.alpha

        def a_update(r):
            rc = lib.wh_replay_prio_update(tp, M, uix.data_ptr(), p.data_ptr(), env.stream)
            assert rc == 0

        def b_update(r):
            vec.index_put_((uix,), p)

        say(f"## M = {M}")
        SA, SA2 = "sample+gather (a)  prio_sample + gather(idx)", "sample+gather (a') ReplayBuffer.sample, weights included"
        SB = "sample+gather (b)  torch cumsum + searchsorted + gather(idx)"
        SB2 = "sample+gather (b') (b) plus the same weights in torch"
        UA, UB = "update (a) wh_replay_prio_update", "update (b) torch index_put_"
        med = run([(SA, a_kernels), (SA2, a_buffer), (SB, b_torch), (SB2, b_torch_weights), (UA, a_update),
                   (UB, b_update)], rounds, reps)
        say(f"sample+gather (b) / (a) = {med[SB] / med[SA]:.2f}   (b') / (a') = {med[SB2] / med[SA2]:.2f}   "
            f"update (b) / (a) = {med[UB] / med[UA]:.2f}   "
            f"sample+gather+update (b') / (a') = {(med[SB2] + med[UB]) / (med[SA2] + med[UA]):.2f}")
    if steps:
        env2 = warehouse.BatchedWarehouse(variant, B, na, seed=3, device=dev)
        env2.reset()
        plain = warehouse.ReplayBuffer(env2, cap)
        acts = env.policy("greedy", 0.1).clone()
        say("## recording")
        med = run([("ReplayBuffer.step, prioritized=True", lambda r: buf.step(acts)),
                   ("ReplayBuffer.step, prioritized=False", lambda r: plain.step(acts))], rounds, reps)
        a, b = med["ReplayBuffer.step, prioritized=True"], med["ReplayBuffer.step, prioritized=False"]
        say(f"prioritized / plain = {a / b:.3f}  (+{a - b:.2f} us per recorded step)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="a rehearsal at toy sizes")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "prio_probe measures on the MI355X: no GPU, no numbers"
    say(f"# {nat.lib().wh_version().decode()}  {torch.cuda.get_device_name(0)}")
    if a.small:
        probe("medium", 8, 1024, 4, (64, 512), 2, 3)
    else:
        probe("medium", 8, 65536, 16, (64, 32768), a.rounds, a.reps)
        probe("medium", 8, 65536, 200, (64, 32768), a.rounds, a.reps, steps=False)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
