"""wh_mlp_forward_multi / warehouse.forward_many / SACCritic(fused=...) on the GPU: several networks of
one shape in ONE launch write byte for byte what the one-network entry points write for the same
arguments.  Every comparison is torch.equal on logits and actions (tests/mlp_multi_cases.py); there
are no tolerances -- rows are independent, the sampler's philox is keyed by the absolute row, and a
job's blocks walk its tasks exactly as a launch of its own would, only with a job-local stride."""
import os
import subprocess
import sys

import pytest

import mlp_multi_cases as mc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def wh():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    import warehouse
    import warehouse.policy  # noqa: F401
    import warehouse.sac  # noqa: F401

    return warehouse


@pytest.fixture(scope="module")
def ops(wh):
    """operands(variant, rows), computed once per shape and shared (never written)."""
    cache = {}

    def get(variant, rows):
        if (variant, rows) not in cache:
            cache[(variant, rows)] = mc.operands(wh, variant, rows, seed=rows)
        return cache[(variant, rows)]

    return get


@pytest.mark.parametrize("variant", ["small", "medium", "large"])
def test_ragged_jobs_guards_and_an_empty_job_between(wh, ops, variant):
    import torch

    specs = mc.ragged_specs(wh, variant, ops)
    assert mc.run_and_compare(wh, specs) == 5
    # the same with a rows = 0 job between live ones: its buffers stay untouched, the others' bytes too
    dead_l, dead_a = mc.Guarded((4, 9), torch.float32), mc.Guarded((4,), torch.int32)
    obs, _ = ops(variant, 1)
    dead = dict(net=specs[0]["net"], obs=obs[:0], logits=dead_l.t[:0], actions=dead_a.t[:0], step=0)
    live = [dict({k: v for k, v in s.items() if k != "want"}, step=s.get("step", 0), logits=True, actions=True)
            for s in specs]
    res = wh.forward_many(live[:2] + [dead] + live[2:])
    assert len(res) == 6 and dead_l.untouched() and dead_a.untouched()
    for s, (a, l) in zip(specs, res[:2] + res[3:]):
        ra, rl = mc.reference(s["net"], dict(s, step=s.get("step", 0)))
        assert torch.equal(a, ra) and torch.equal(l, rl)


@pytest.mark.parametrize("variant", ["medium", "small"])
def test_over_the_cap_blocks_walk_several_tasks_with_a_job_local_stride(wh, ops, variant):
    """Three jobs of 30,725 rows: 3 x 121 = 363 tasks of 256 rows on (at most) 256 CUs, so the blocks of
    every job take a second task -- it > 0, the next-task operand load of k_mlp16 (Medium) and the X
    prefetch of k_mlp (Small) -- with the job's own stride and a ragged last task."""
    import torch

    rows = 30_725
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert 3 * ((rows + 255) // 256) > cus, cus
    obs, xf = ops(variant, rows)
    nets = [wh.policy.MLPPolicy(variant, seed=60 + i) for i in range(3)]
    specs = [dict(net=nets[0], obs=obs), dict(net=nets[1], xfrag=xf, rows=rows, explore=True, seed=3, step=5),
             dict(net=nets[2], obs=obs, explore=True, seed=4, step=6)]
    assert mc.run_and_compare(wh, specs) == 3


@pytest.mark.parametrize("njobs", [1, 8])
def test_job_count_limits(wh, ops, njobs):
    rows = (203, 1, 257, 256, 1, 203, 257, 700)[:njobs]
    nets = [wh.policy.MLPPolicy("medium", seed=70 + i) for i in range(njobs)]
    specs = []
    for i, (r, net) in enumerate(zip(rows, nets)):
        obs, xf = ops("medium", r)
        specs.append(dict(net=net, obs=obs) if i % 2 else dict(net=net, xfrag=xf, rows=r))
    assert mc.run_and_compare(wh, specs) == njobs
    with pytest.raises(ValueError, match="at most 8"):
        wh.forward_many([dict(s, logits=True) for s in specs] * 9)


@pytest.mark.parametrize("variant", ["small", "medium", "large"])
def test_f32_precision(wh, ops, variant):
    """The f32 kernel's grid is not persistent: four 32-row waves per block, a job's last block partly
    idle (rows 31: one wave; 128: exactly one block; 300: three blocks, the last with two waves)."""
    rows = (31, 128, 300)
    nets = [wh.policy.MLPPolicy(variant, seed=80 + i, precision="f32") for i in range(3)]
    specs = [dict(net=n, obs=ops(variant, 700)[0][:r].contiguous()) for r, n in zip(rows, nets)]
    specs[1].update(explore=True, seed=2, step=1)
    assert mc.run_and_compare(wh, specs) == 3
    with pytest.raises(ValueError, match="bf16"):
        wh.forward_many([dict(net=nets[0], xfrag=ops(variant, 700)[1], rows=700, logits=True)])


def test_legacy_route_in_a_fresh_process():
    """bf16 Medium with WH_MLP_LEGACY=1 (k_mlp on 32x32x16 tiles): the choice is a process-wide static,
    so a fresh child process runs the ragged case there."""
    env = dict(os.environ, WH_MLP_LEGACY="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mlp_multi_cases.py")], capture_output=True,
                       text=True, env=env, timeout=120)
    assert r.returncode == 0 and "LEGACY MULTI OK 5" in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_non_default_stream(wh, ops):
    import torch

    specs = mc.ragged_specs(wh, "medium", ops)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        jobs = [dict({k: v for k, v in s.items() if k != "want"}, step=s.get("step", 0), logits=True, actions=True)
                for s in specs]
        got = wh.forward_many(jobs)
    side.synchronize()
    for s, (a, l) in zip(specs, got):
        ra, rl = mc.reference(s["net"], dict(s, step=s.get("step", 0)))
        assert torch.equal(a, ra) and torch.equal(l, rl)


def test_forward_many_refuses_mixed_networks_and_takes_the_networks_own_step(wh, ops):
    import torch

    obs, xf = ops("medium", 203)
    bf, f32 = wh.policy.MLPPolicy("medium", seed=1), wh.policy.MLPPolicy("medium", seed=1, precision="f32")
    with pytest.raises(ValueError, match="share shape, precision"):
        wh.forward_many([dict(net=bf, obs=obs), dict(net=f32, obs=obs)])
    with pytest.raises(ValueError, match="share shape, precision"):
        wh.forward_many([dict(net=bf, obs=obs), dict(net=wh.policy.MLPPolicy("small", seed=1), obs=ops("small", 1)[0])])
    with pytest.raises(ValueError, match="either"):
        wh.forward_many([dict(net=bf, obs=obs, xfrag=xf, rows=203)])
    # a later job's defect leaves the earlier jobs' counters alone: nothing was launched
    with pytest.raises(ValueError, match="either"):
        wh.forward_many([dict(net=bf, obs=obs), dict(net=bf, obs=obs, xfrag=xf, rows=203)])
    assert bf._step == 0
    # step=None takes (and advances) each network's own counter, as forward() does
    twin = wh.policy.MLPPolicy("medium", seed=1)
    for _ in range(2):
        (a, none), = wh.forward_many([dict(net=bf, obs=obs, explore=True, seed=9)])
        ra, _ = twin.forward(obs, explore=True, seed=9)
        assert none is None and torch.equal(a, ra)
    assert bf._step == twin._step == 2
    # logits asked for and no actions: none computed, none returned
    (a, l), = wh.forward_many([dict(net=bf, obs=obs, logits=True)])
    assert a is None and torch.equal(l, twin.forward(obs, logits=True)[1])


# ----------------------------------------------------------------------------- SACCritic
def sac_batch(wh, variant, B, NA, M, seed):
    import numpy as np

    env = wh.BatchedWarehouse(variant, B, NA, seed=seed, device="cuda:0")
    env.reset()
    buf = wh.ReplayBuffer(env, capacity=4, prioritized=True)
    for _ in range(4):
        buf.step(env.policy("greedy", 0.3))
    idx = np.random.default_rng(seed).integers(0, len(buf), M)
    return {k: v.clone() for k, v in buf.sample(M, idx=idx, rows=False, fragments=True).items()}


@pytest.mark.parametrize("variant,NA,M", [("medium", 8, 64), ("medium", 9, 3)])
@pytest.mark.parametrize("twin", [True, False])
def test_critic_fused_equals_sequential_bit_for_bit(wh, variant, NA, M, twin):
    import torch

    batch = sac_batch(wh, variant, 16, NA, M, seed=21)
    nets = [wh.policy.MLPPolicy(variant, seed=90 + i) for i in range(5)]
    if not twin:
        nets[2] = nets[4] = None
    seq = wh.SACCritic(*nets, alpha=0.2, gamma=0.97, fused=False)
    fus = wh.SACCritic(*nets, alpha=0.2, gamma=0.97, fused=True)
    auto = wh.SACCritic(*nets, alpha=0.2, gamma=0.97)
    want = {k: v.clone() for k, v in seq.td(batch).items()}
    assert seq.last_fused is False
    got = fus.td(batch)
    assert fus.last_fused is True and set(got) == {"y", "td_rows", "td"}
    for k in want:
        assert torch.equal(got[k], want[k]), k
    assert float(want["td"].abs().max()) > 0
    # targets: three forwards, the same y
    assert torch.equal(fus.targets(batch)["y"], want["y"]) and torch.equal(seq.targets(batch)["y"], want["y"])
    # out= buffers are the caller's on the fused route too
    mine = dict(y=torch.full((M, NA), -1.0, device="cuda:0"), td=torch.full((M,), -1.0, device="cuda:0"))
    res = fus.td(batch, out=mine)
    assert res["y"].data_ptr() == mine["y"].data_ptr() and torch.equal(mine["y"], want["y"]) and torch.equal(mine["td"], want["td"])
    # auto: these batches are far below the row threshold
    assert M * NA <= wh.sac.FUSED_MAX_ROWS and auto.use_fused(M * NA) and not auto.use_fused(wh.sac.FUSED_MAX_ROWS + 1)
    res = auto.td(batch)
    assert auto.last_fused is True and all(torch.equal(res[k], want[k]) for k in want)


def test_critic_fused_needs_one_shape(wh):
    bf = [wh.policy.MLPPolicy("small", seed=i) for i in range(3)]
    f32 = wh.policy.MLPPolicy("small", seed=4, precision="f32")
    with pytest.raises(ValueError, match="one shape and precision"):
        wh.SACCritic(bf[0], bf[1], None, f32, None, alpha=0.2, fused=True)
    mixed = wh.SACCritic(bf[0], bf[1], None, f32, None, alpha=0.2)      # auto: sequential
    assert mixed.one_shape is False and mixed.use_fused(8) is False
