"""The SAC forward half on the card: the device weight repack against the host route it replaces, and
the TD epilogue against the same formula as torch ops, in one process.

    python tools/sac_probe.py [--out profiles/sac_probe.txt] [--rounds 5]

Every variant is warmed up; variants are interleaved per round; device times are HIP events over
`reps` back-to-back calls (median [min .. max] over the rounds).

  pack, per variant (small / medium / large) and precision (bf16 / f32)
    (a)  MLPPolicy.load_weights from six device tensors: wh_mlp_pack_device, one launch (events)
    (a') the same, wall clock from before the call to after a stream synchronize
    (b)  the host route, the only one before wh_mlp_pack_device: .cpu() of the six tensors, then
         wh_mlp_pack (CPU pack + a synchronous host-to-device copy); wall clock from before the
         copies to after the call returns
  TD epilogue, Medium-8, M = 64 (the YAMLs' train_batch_size) and M = 32,768
    (a)  wh_sac_td on five [M*8, 9] logit tensors: one launch
    (b)  the same formula as torch ops on the same tensors (the op count is printed)
    and SACCritic.td on a sampled fragment batch: the five forwards alone, the epilogue alone, and
    the whole call (the sequential route, fused=False); the epilogue's bytes moved against the 8 TB/s
    HBM figure bench.py uses
  one launch for the five forwards (wh_mlp_forward_multi), Medium-8, M = 64 and M = 32,768 (--fused-m
  for other batch sizes)
    the five forwards alone and the whole SACCritic.td, fused=True against fused=False, interleaved.
    A library without the entry point (the parent commit's, loaded with WAREHOUSE_AMD_LIB and
    WAREHOUSE_AMD_AB=1 for a side-by-side run) measures the sequential route alone.
    --only fused runs just this section
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rllib-warehouse_amd")]

import torch  # noqa: E402
from torch.utils._python_dispatch import TorchDispatchMode  # noqa: E402

import warehouse  # noqa: E402
from warehouse import _native as nat  # noqa: E402
from warehouse.policy import MLPPolicy, init_weights  # noqa: E402

HBM_PEAK = 8.0e12
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


def wall_us(fn, reps):
    """Host wall clock per call; `fn` itself ends synchronised."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for r in range(reps):
        fn(r)
    return (time.perf_counter() - t0) / reps * 1e6


def report(name, samples):
    med = statistics.median(samples)
    say(f"{name:72s} {med:10.2f} us  [{min(samples):.2f} .. {max(samples):.2f}]")
    return med


def run(variants, rounds, reps):
    """variants: (name, fn, timer).  Warm up, then interleave per round."""
    for _, fn, _ in variants:
        for r in range(3):
            fn(r)
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in variants}
    for _ in range(rounds):
        for name, fn, timer in variants:
            times[name].append(timer(fn, reps))
    return {name: report(name, times[name]) for name, _, _ in variants}


def probe_pack(rounds, reps):
    say("# pack: MLPPolicy.load_weights(device tensors) against .cpu() + wh_mlp_pack")
    fp = ctypes.POINTER(ctypes.c_float)
    keys = ("w0", "b0", "w1", "b1", "w2", "b2")
    for variant in ("small", "medium", "large"):
        for precision in ("bf16", "f32"):
            net = MLPPolicy(variant, seed=1, device=DEV, precision=precision)
            w = init_weights(net.in_dim, *net.hidden, seed=2)
            wd = {k: torch.as_tensor(w[k]).to(DEV).contiguous() for k in keys}
            f32_bytes = sum(v.numel() for v in wd.values()) * 4

            def device_route(r):
                net.load_weights(wd)

            def device_route_wall(r):
                net.load_weights(wd)
                torch.cuda.current_stream().synchronize()

            def host_route(r):
                h = {k: wd[k].cpu().numpy() for k in keys}
                with torch.cuda.device(DEV):
                    rc = nat.lib().wh_mlp_pack(ctypes.byref(net.desc), *[h[k].ctypes.data_as(fp) for k in keys],
                                               net.packed.data_ptr())
                assert rc == 0

            say(f"## {variant} {precision}: {f32_bytes / 1e3:.0f} KB of f32 weights -> a {net.packed.numel() / 1e3:.0f} KB blob")
            A, A2, B = "(a)  load_weights, device tensors (events)", "(a') load_weights + stream sync (wall clock)", \
                "(b)  .cpu() x 6 + wh_mlp_pack (wall clock)"
            med = run([(A, device_route, time_us), (A2, device_route_wall, wall_us), (B, host_route, wall_us)], rounds, reps)
            say(f"(b) / (a') = {med[B] / med[A2]:.1f}   (b) / (a) = {med[B] / med[A]:.1f}")


class OpCounter(TorchDispatchMode):
    """Dispatched aten ops that launch a kernel (views and metadata ops left out)."""
    VIEWS = {"view", "reshape", "squeeze", "unsqueeze", "expand", "alias", "detach", "select", "slice", "_unsafe_view"}

    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if func._schema.name.split("::")[-1] not in self.VIEWS:
            self.n += 1
        return func(*args, **(kwargs or {}))


def torch_td(pi, q1t, q2t, q1, q2, actions, rewards, n, alpha, discount, M, NA):
    """The formula of include/warehouse_amd.h (SAC TD TARGETS) as torch ops, mask_dones = 0."""
    logp = torch.log_softmax(pi, 1)
    v = (logp.exp() * (torch.minimum(q1t, q2t) - alpha * logp)).sum(1)
    live = (torch.arange(NA, device=pi.device)[None, :] < n[:, None]).reshape(-1)
    y = torch.where(live, rewards.reshape(-1) + discount * v, 0.0)
    a = torch.where((actions >= 0) & (actions < 9), actions, 4).reshape(-1, 1).long()
    td_rows = 0.5 * ((q1.gather(1, a).squeeze(1) - y).abs() + (q2.gather(1, a).squeeze(1) - y).abs())
    td_rows = torch.where(live, td_rows, 0.0)
    td = td_rows.view(M, NA).sum(1) / n.clamp(min=1)
    td = torch.where(n > 0, td, 0.0)
    return y.view(M, NA), td_rows.view(M, NA), td


def probe_td(rounds, reps):
    NA = 8
    env = warehouse.BatchedWarehouse("medium", 4096, NA, seed=3, device=DEV)
    env.reset()
    buf = warehouse.ReplayBuffer(env, 16)
    for _ in range(16):
        buf.step(env.policy("greedy", 0.1), observe=False)
    nets = [MLPPolicy("medium", seed=10 + i, device=DEV) for i in range(5)]
    critic = warehouse.SACCritic(*nets, alpha=0.2, gamma=0.99, fused=False)
    g = torch.Generator(device=DEV).manual_seed(7)
    for M in (64, 32768):
        rows = M * NA
        lg = [(torch.rand((rows, 9), device=DEV, generator=g) * 2 - 1) * s for s in (4, 10, 10, 10, 10)]
        actions = torch.randint(0, 9, (M, NA), device=DEV, generator=g, dtype=torch.int32)
        rewards = torch.randint(-1, 2, (M, NA), device=DEV, generator=g).float()
        n = torch.full((M,), NA, dtype=torch.int32, device=DEV)
        y, tr, td = (torch.empty((M, NA), device=DEV), torch.empty((M, NA), device=DEV), torch.empty(M, device=DEV))
        args = nat.WhSacTdArgs(*[t.data_ptr() for t in lg], actions.data_ptr(), rewards.data_ptr(), None, n.data_ptr(),
                               0.2, 0.99, 0, y.data_ptr(), tr.data_ptr(), td.data_ptr())
        stream = nat.stream_of(DEV)

        def a_kernel(r):
            assert nat.lib().wh_sac_td(M, NA, ctypes.byref(args), stream) == 0

        def b_torch(r):
            torch_td(*lg, actions, rewards, n, 0.2, 0.99, M, NA)

        with OpCounter() as oc:
            want = torch_td(*lg, actions, rewards, n, 0.2, 0.99, M, NA)
        a_kernel(0)
        torch.cuda.synchronize()
        err = max(float((a - b).abs().max()) for a, b in zip((y, tr, td), want))
        batch = buf.sample(M, draw=1, rows=False, fragments=True)

        def forwards(r):
            for net, side, name in zip(nets, ("next_", "next_", "next_", "", ""), ("pi_next", "q1t_next", "q2t_next", "q1", "q2")):
                critic._forward(net, batch, side, rows, name)

        def whole(r):
            critic.td(batch)

        moved = rows * 9 * 4 * 5 + rows * 8 + M * 4 + rows * 8 + M * 4
        say(f"## TD epilogue, Medium-8, M = {M} ({rows} rows, {moved / 1e6:.2f} MB moved); wh_sac_td vs torch: max |diff| {err:.2e}")
        KA, KB = "(a)  wh_sac_td: 1 launch", f"(b)  torch ops: {oc.n} launches"
        F, W = "SACCritic.td: the five forwards alone", "SACCritic.td: the whole call"
        med = run([(KA, a_kernel, time_us), (KB, b_torch, time_us), (F, forwards, time_us), (W, whole, time_us)], rounds, reps)
        say(f"(b) / (a) = {med[KB] / med[KA]:.1f}   epilogue share of SACCritic.td = {med[KA] / med[W]:.3f}   "
            f"forwards share = {med[F] / med[W]:.3f}   epilogue {moved / (med[KA] * 1e-6) / 1e12:.3f} TB/s = "
            f"{moved / (med[KA] * 1e-6) / HBM_PEAK:.3f} of the 8 TB/s HBM peak")


def probe_fused(rounds, reps, Ms):
    NA = 8
    env = warehouse.BatchedWarehouse("medium", 4096, NA, seed=3, device=DEV)
    env.reset()
    buf = warehouse.ReplayBuffer(env, 16)
    for _ in range(16):
        buf.step(env.policy("greedy", 0.1), observe=False)
    nets = [MLPPolicy("medium", seed=10 + i, device=DEV) for i in range(5)]
    have = hasattr(nat.lib(), "wh_mlp_forward_multi")
    seq = warehouse.SACCritic(*nets, alpha=0.2, gamma=0.99, fused=False)
    fus = warehouse.SACCritic(*nets, alpha=0.2, gamma=0.99, fused=True) if have else None
    say("# five forwards in one launch (wh_mlp_forward_multi) against five launches, Medium-8" +
        ("" if have else "  -- this library lacks the entry point: the sequential route alone"))
    for M in Ms:
        rows = M * NA
        batch = buf.sample(M, draw=1, rows=False, fragments=True)

        def fwd_seq(r):
            for net, side, name in zip(nets, ("next_", "next_", "next_", "", ""), ("pi_next", "q1t_next", "q2t_next", "q1", "q2")):
                seq._forward(net, batch, side, rows, name)

        def fwd_fus(r):
            fus._forward_fused(batch, rows, True)

        def td_seq(r):
            seq.td(batch)

        def td_fus(r):
            fus.td(batch)

        say(f"## Medium-8, M = {M} ({rows} agent rows, {(rows + 255) // 256} tasks per network)")
        FS, FF = "the five forwards alone, sequential (5 launches)", "the five forwards alone, fused (1 launch)"
        TS, TF = "SACCritic.td, fused=False (6 launches)", "SACCritic.td, fused=True (2 launches)"
        variants = [(FS, fwd_seq, time_us), (TS, td_seq, time_us)]
        if have:
            want = {k: v.clone() for k, v in seq.td(batch).items()}
            got = fus.td(batch)
            assert all(torch.equal(got[k], want[k]) for k in want), "the two routes differ"
            variants = [(FS, fwd_seq, time_us), (FF, fwd_fus, time_us), (TS, td_seq, time_us), (TF, td_fus, time_us)]
        med = run(variants, rounds, reps)
        if have:
            say(f"forwards sequential / fused = {med[FS] / med[FF]:.2f}   td sequential / fused = {med[TS] / med[TF]:.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=("all", "fused"), default="all")
    ap.add_argument("--fused-m", type=int, nargs="+", default=[64, 32768])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "sac_probe measures on the MI355X: no GPU, no numbers"
    say(f"# {nat.lib().wh_version().decode()}  {torch.cuda.get_device_name(0)}")
    if a.only == "all":
        probe_pack(a.rounds, a.reps)
        probe_td(a.rounds, a.reps)
    probe_fused(a.rounds, a.reps, a.fused_m)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
