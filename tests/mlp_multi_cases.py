"""Cases of wh_mlp_forward_multi / warehouse.forward_many, shared by tests/test_gpu_mlp_multi.py and its
WH_MLP_LEGACY child process (this file run as a program).  Every comparison is torch.equal -- bytes --
against the one-network entry points (MLPPolicy.forward / forward_x) on the same inputs: no tolerance.

Inputs are real observation rows: a BatchedWarehouse of `rows` one-agent envs after a short greedy
rollout gives the f32 rows and, from observe_x, the same rows as the fragment-order operand."""
import numpy as np

GUARD = 256      # bytes around every output
FILL = 0x5A


def operands(wh, variant, rows, seed):
    """(obs [rows, 9R+1] f32, xfrag) of `rows` observation rows, both cloned off the env."""
    env = wh.BatchedWarehouse(variant, rows, 1, seed=seed, device="cuda:0")
    env.reset()
    env.rollout(5, "greedy", 0.1)
    xf, obs = env.observe_x(obs=True)
    return obs.reshape(rows, env.obs_len).clone(), xf.clone()


class Guarded:
    """A [shape] tensor of `dtype` inside a byte buffer with GUARD bytes of FILL on either side (the
    payload is FILL too, so an untouched output is recognisable)."""

    def __init__(self, shape, dtype):
        import torch

        n = int(np.prod(shape)) * 4
        self.raw = torch.full((GUARD + n + GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
        self.t = self.raw[GUARD:GUARD + n].view(dtype).view(shape)

    def guards_intact(self):
        return bool((self.raw[:GUARD] == FILL).all()) and bool((self.raw[-GUARD:] == FILL).all())

    def untouched(self):
        return bool((self.raw == FILL).all())


def reference(net, spec):
    """What the one-network entry point writes for this job: (actions, logits)."""
    kw = dict(explore=spec.get("explore", False), seed=spec.get("seed", 0), step=spec.get("step", 0), logits=True)
    if "xfrag" in spec:
        return net.forward_x(spec["xfrag"], spec["rows"], **kw)
    return net.forward(spec["obs"], **kw)


def run_and_compare(wh, specs, want=("logits", "actions")):
    """forward_many over `specs` (dicts with net, obs | xfrag + rows, explore / seed / step, and
    optionally want=...) into guarded buffers, against reference() job by job.  Returns the number
    of jobs compared."""
    import torch

    jobs, outs = [], []
    for s in specs:
        rows = s["rows"] if "xfrag" in s else s["obs"].shape[0]
        w = s.get("want", want)
        lg = Guarded((rows, 9), torch.float32) if "logits" in w else None
        ac = Guarded((rows,), torch.int32) if "actions" in w else None
        j = {k: v for k, v in s.items() if k != "want"}
        j.setdefault("step", 0)
        if lg is not None:
            j["logits"] = lg.t
        if ac is not None:
            j["actions"] = ac.t
        jobs.append(j)
        outs.append((ac, lg))
    res = wh.forward_many(jobs)
    assert len(res) == len(specs)
    for s, (ac, lg), (ra, rl) in zip(specs, outs, res):
        assert (ra is None) == (ac is None) and (rl is None) == (lg is None)
        ref_a, ref_l = reference(s["net"], dict(s, step=s.get("step", 0)))
        if lg is not None:
            assert rl.data_ptr() == lg.t.data_ptr()
            assert torch.equal(lg.t, ref_l), "logits differ from the one-network launch"
            assert lg.guards_intact()
        if ac is not None:
            assert ra.data_ptr() == ac.t.data_ptr()
            assert torch.equal(ac.t, ref_a), "actions differ from the one-network launch"
            assert ac.guards_intact()
    return len(specs)


def ragged_specs(wh, variant, ops):
    """Five jobs of rows (1, 203, 256, 257, 700) -- a partial task, a partial task of several waves,
    exactly one task, one task plus a row, several tasks -- alternating obs / xfrag, each with its own
    weights; two explore with different seed / step; one logits only, one actions only."""
    rows = (1, 203, 256, 257, 700)
    nets = [wh.policy.MLPPolicy(variant, seed=40 + i) for i in range(5)]
    specs = []
    for i, (r, net) in enumerate(zip(rows, nets)):
        obs, xf = ops(variant, r)
        s = dict(net=net, xfrag=xf, rows=r) if i % 2 else dict(net=net, obs=obs)
        specs.append(s)
    specs[1].update(explore=True, seed=7, step=3)
    specs[4].update(explore=True, seed=(5 << 32) | 9, step=11)
    specs[2]["want"] = ("logits",)
    specs[3]["want"] = ("actions",)
    return specs


if __name__ == "__main__":   # the WH_MLP_LEGACY child of tests/test_gpu_mlp_multi.py: Medium on the 32x32x16 kernel
    import os
    import sys

    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [ROOT, os.path.join(ROOT, "rllib-warehouse_amd")]
    import warehouse
    import warehouse.policy  # noqa: F401

    assert os.environ.get("WH_MLP_LEGACY") == "1"
    cache = {}

    def ops(variant, rows):
        if (variant, rows) not in cache:
            cache[(variant, rows)] = operands(warehouse, variant, rows, seed=rows)
        return cache[(variant, rows)]

    print("LEGACY MULTI OK", run_and_compare(warehouse, ragged_specs(warehouse, "medium", ops)))
