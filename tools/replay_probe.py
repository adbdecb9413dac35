"""Replay gather against the routes it replaces, on the card, in one process.

    python tools/replay_probe.py [--out profiles/replay_probe.txt] [--rounds 5]

Medium-8, B = 65,536, capacity 16: a 278 MB ring (beyond the Infinity Cache).  M = 32,768 samples
with device-drawn indices, so one gather writes the 172 MB of rows one wh_observe of the full batch
writes.  Output buffers rotate, so rows go to fresh memory.  Variants, interleaved per round and
timed with HIP events (median and spread over the rounds):

  (a)  wh_replay_gather: obs + next_obs rows; then xfrag + next_xfrag only
  (b)  what a user has without the ring: plane-major state snapshots kept per step,
       torch.index_select of the sampled envs into two [words, M] buffers, two wh_observe calls
  (c)  one wh_observe of 65,536 contiguous envs: the row writer's own ceiling for these bytes

then ReplayBuffer.step against vector_step(autoreset=True) per step, and one Large-16 line of (a)
against (c).  --gather-only launches (a) rows alone, for a counter pass of its own:
    rocprofv3 --pmc FETCH_SIZE -T --output-format csv -d DIR -o run -- python3 tools/replay_probe.py --gather-only
Algorithmic bytes of a gather: the rows (or fragments) written plus 2 M records read.

--only record times the recorded step alone: ReplayBuffer.step with fused=False (put,
step, put, reset, observe), with fused=True (wh_replay_record + observe) and vector_step(autoreset=True),
then collect(5) against 5 x step, each with f32 rows and with the fragment operand, at Medium-8
B = 65,536 / 4,096 / 256 and Large-16 B = 65,536.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rllib-warehouse_amd")]

import torch  # noqa: E402

import warehouse  # noqa: E402

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


def report(name, samples, nbytes=None):
    med = statistics.median(samples)
    rate = f"  {nbytes / med / 1e3:8.1f} GB/s ({nbytes / 1e6:.1f} MB)" if nbytes else ""
    say(f"{name:58s} {med:9.2f} us  [{min(samples):.2f} .. {max(samples):.2f}]{rate}")
    return med


def probe(variant, na, B, cap, M, rounds, reps, baseline=True, NBUF=3, gather_only=False):
    dev = torch.device("cuda", 0)
    env = warehouse.BatchedWarehouse(variant, B, na, seed=3, device=dev)
    env.reset()
    env.stagger(torch.arange(B, device=dev) % 7)
    buf = warehouse.ReplayBuffer(env, cap)
    snaps = []                                              # route (b)'s storage: plane-major snapshots
    for s in range(cap):
        pre = env.state.clone()
        buf.step(env.policy("greedy", 0.1), observe=False)
        snaps.append(pre)
    words, L = env.layout.words_per_env, env.obs_len
    rec_bytes = 2 * M * words * 4
    rows_bytes = 2 * M * na * L * 4
    ring_mb = sum(t.numel() * t.element_size() for t in (buf.states, buf.actions, buf.rewards, buf.dones)) / 1e6
    say(f"# {variant}-{na}  B = {B}  capacity = {cap} (ring {ring_mb:.0f} MB)  M = {M}  "
        f"record {words * 4} B  rows of a gather {rows_bytes / 1e6:.1f} MB")
    shapes = buf._shapes(M)
    outs = [{k: torch.empty(shapes[k][0], dtype=shapes[k][1], device=dev) for k in
             ("obs", "next_obs", "actions", "rewards", "dones", "n", "idx_out")} for _ in range(NBUF)]
    fouts = [{k: torch.empty(shapes[k][0], dtype=shapes[k][1], device=dev) for k in
              ("xfrag", "next_xfrag", "actions", "rewards", "dones", "n", "idx_out")} for _ in range(NBUF)]
    frag_bytes = 2 * fouts[0]["xfrag"].numel()

    def a_rows(r):
        buf.sample(M, draw=r, out=outs[r % NBUF])

    def a_frags(r):
        buf.sample(M, draw=r, out=fouts[r % NBUF])

    if gather_only:                                         # a counter pass (rocprofv3 --pmc): (a) rows alone
        for r in range(12):
            a_rows(r)
        torch.cuda.synchronize()
        return

    # (b): the sampled envs of one snapshot pair -> [words, M] x 2 -> two wh_observe of M envs
    twin = warehouse.BatchedWarehouse(variant, M, na, seed=3, device=dev)
    sel = torch.randint(0, B, (M,), device=dev)
    stage = [torch.empty((words, M), dtype=torch.int32, device=dev) for _ in range(2)]
    brows = [[torch.empty((M, na, L), dtype=torch.float32, device=dev) for _ in range(2)] for _ in range(NBUF)]
    cfgp, lib = twin._cfgp, twin._lib

    def b_route(r):
        s = r % (cap - 1)
        for side in range(2):
            torch.index_select(snaps[s + side], 1, sel, out=stage[side])
            rc = lib.wh_observe(cfgp, M, stage[side].data_ptr(), brows[r % NBUF][side].data_ptr(), twin.stream)
            assert rc == 0

    # (c): wh_observe of B contiguous envs (2 M = B: the same rows)
    crows = [torch.empty((B, na, L), dtype=torch.float32, device=dev) for _ in range(NBUF)]

    def c_observe(r):
        rc = env._lib.wh_observe(env._cfgp, B, env.state.data_ptr(), crows[r % NBUF].data_ptr(), env.stream)
        assert rc == 0

    acts = env.policy("greedy", 0.1).clone()

    def step_buf(r):
        buf.step(acts)

    def step_plain(r):
        env.vector_step(acts, autoreset=True)

    variants = [("(a) wh_replay_gather rows", a_rows, rows_bytes + rec_bytes),
                ("(a) wh_replay_gather fragments only", a_frags, frag_bytes + rec_bytes)]
    if baseline:
        variants += [("(b) index_select x2 + wh_observe x2", b_route, None)]
    variants += [(f"(c) wh_observe of {B} contiguous envs", c_observe, crows[0].numel() * 4 + env.state.numel() * 4)]
    if baseline:
        variants += [("ReplayBuffer.step (put, step, put, reset, observe)", step_buf, None),
                     ("vector_step(autoreset=True)", step_plain, None)]
    for _, fn, _ in variants:                               # warm-up: every variant, every buffer
        for r in range(2 * NBUF):
            fn(r)
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in variants}
    for _ in range(rounds):                                 # interleaved
        for name, fn, _ in variants:
            times[name].append(time_us(fn, reps))
    med = {name: report(name, times[name], nb) for name, _, nb in variants}
    a, c = med["(a) wh_replay_gather rows"], med[f"(c) wh_observe of {B} contiguous envs"]
    say(f"(a) / (c) = {a / c:.3f}")
    if baseline:
        say(f"(b) / (a) = {med['(b) index_select x2 + wh_observe x2'] / a:.3f}")
        say(f"ReplayBuffer.step / vector_step = "
            f"{med['ReplayBuffer.step (put, step, put, reset, observe)'] / med['vector_step(autoreset=True)']:.3f}")


def probe_record(variant, na, B, rounds, reps, cap=8):
    """The recorded step's routes at one shape: three envs in one state, one buffer per route."""
    dev = torch.device("cuda", 0)
    envs = [warehouse.BatchedWarehouse(variant, B, na, seed=3, device=dev) for _ in range(3)]
    for e in envs:
        e.reset()
        e.stagger(torch.arange(B, device=dev) % 7)
    unfused = warehouse.ReplayBuffer(envs[0], cap, fused=False)
    fused = warehouse.ReplayBuffer(envs[1], cap, fused=True)
    plain = envs[2]
    acts = plain.policy("greedy", 0.1).clone()
    ring_mb = sum(t.numel() * t.element_size() for t in (fused.states, fused.actions, fused.rewards, fused.dones)) / 1e6
    say(f"# record: {variant}-{na}  B = {B}  capacity = {cap} (ring {ring_mb:.1f} MB)  "
        f"record writes of a step {2 * B * envs[0].layout.words_per_env * 4 / 1e6:.2f} MB")
    for operand in ("rows", "fragments"):
        step_x = plain.vector_step_x if operand == "fragments" else plain.vector_step
        variants = [(f"step fused=False, {operand}", lambda r: unfused.step(acts, operand=operand)),
                    (f"step fused=True, {operand}", lambda r: fused.step(acts, operand=operand)),
                    (f"vector_step(autoreset=True), {operand}", lambda r: step_x(acts, autoreset=True)),
                    (f"5 x step fused=False + policy, {operand}",
                     lambda r: [unfused.step(envs[0].policy("greedy", 0.1), operand=operand) for _ in range(5)]),
                    (f"collect(5) fused=True, {operand}", lambda r: fused.collect(5, "greedy", 0.1, operand=operand))]
        for _, fn in variants:
            for r in range(4):
                fn(r)
        torch.cuda.synchronize()
        times = {name: [] for name, _ in variants}
        for _ in range(rounds):                             # interleaved
            for name, fn in variants:
                times[name].append(time_us(fn, reps if "5" not in name.split(",")[0] else max(reps // 5, 4)))
        med = {name: report(name, times[name]) for name, _ in variants}
        names = [n for n, _ in variants]
        bar = min(times[names[0]])
        say(f"fused / unfused = {med[names[1]] / med[names[0]]:.3f}   fused / vector_step = {med[names[1]] / med[names[2]]:.3f}   "
            f"fused median {'below' if med[names[1]] < bar else 'NOT below'} the unfused minimum {bar:.2f}")
        say(f"collect(5) / 5 x step = {med[names[4]] / med[names[3]]:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--small", action="store_true", help="a rehearsal at toy sizes")
    ap.add_argument("--only", choices=["record"], default=None, help="record: the recorded step's routes alone")
    ap.add_argument("--gather-only", action="store_true",
                    help="12 launches of (a) rows at the Medium-8 shape and nothing else: the run a counter pass wraps")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "replay_probe measures on the MI355X: no GPU, no numbers"
    from warehouse import _native

    say(f"# {_native.lib().wh_version().decode()}  {torch.cuda.get_device_name(0)}")
    if a.only == "record":
        if a.small:
            probe_record("medium", 8, 300, 2, 5)
            probe_record("large", 16, 100, 2, 5)
        else:
            for B in (65536, 4096, 256):
                probe_record("medium", 8, B, a.rounds, a.reps)
            probe_record("large", 16, 65536, a.rounds, a.reps)
    elif a.gather_only:
        probe("medium", 8, 65536, 16, 32768, 0, 0, gather_only=True)
    elif a.small:
        probe("medium", 8, 1024, 4, 512, 2, 3)
        probe("large", 16, 256, 4, 128, 2, 3, baseline=False)
    else:
        probe("medium", 8, 65536, 16, 32768, a.rounds, a.reps)
        probe("large", 16, 65536, 4, 32768, a.rounds, max(a.reps // 2, 5), baseline=False, NBUF=2)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
