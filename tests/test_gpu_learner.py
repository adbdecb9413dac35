"""warehouse.SACLearner end to end on the GPU: Small-4, B = 8, a wrapped prioritized ring, 16 samples with
duplicates and one planted out-of-ring index, f32 modules and f32 critic networks, a bf16 rollout policy.
One update is taken apart: the d(loss)/d(logits) against float64 torch autograd of the written-out losses
(within the bounds of tests/loss_cases.py), the gradients, the Adam step, the repacked blobs and the target
update bit for bit against the same calls made by hand; a second update on a side stream against one on
the default stream.

Largest d(loss)/d(logits) errors seen against float64 autograd, as fractions of the bounds (dpi, dq1, dq2):
0.0018, 0.079, 0.059."""
import copy

import numpy as np
import pytest

import loss_cases as lc

pytestmark = pytest.mark.gpu

KEYS = ("w0", "b0", "w1", "b1", "w2", "b2")
M, NA = 16, 4
TE = 0.935


@pytest.fixture(scope="module")
def wh():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    import warehouse
    import warehouse.policy  # noqa: F401

    return warehouse


def module(seed):
    import torch

    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(37, 256), torch.nn.ReLU(), torch.nn.Linear(256, 256), torch.nn.ReLU(),
                               torch.nn.Linear(256, 9)).to("cuda:0")


def numpy_weights(wh, mod):
    return {k: v.cpu().numpy() for k, v in wh.policy.weights_of(mod).items()}


@pytest.fixture(scope="module")
def batch(wh):
    """test_gpu_sac.py's ring: 4 slots wrapped by six recorded steps; rows for the f32 networks, and
    importance weights as a prioritized draw would bring."""
    import torch
    from replay_cases import place_near_end

    env = wh.BatchedWarehouse("small", 8, NA, seed=11, device="cuda:0")
    place_near_end(env)
    buf = wh.ReplayBuffer(env, capacity=4, prioritized=True)
    for _ in range(6):
        buf.step(env.policy("greedy", 0.3))
    assert buf.filled == 4 and buf.cursor == 2
    rng = np.random.default_rng(5)
    idx = rng.integers(0, len(buf), M)
    idx[3] = idx[9]
    idx[6] = len(buf) + 7                                     # outside the ring: n = -1
    b = {k: v.clone() for k, v in buf.sample(M, idx=idx, rows=True).items()}
    b["weights"] = torch.as_tensor(rng.choice(np.array([0.25, 0.5, 0.75, 1.0], np.float32), M)).to("cuda:0")
    assert int(b["n"][6]) == -1
    torch.cuda.synchronize()
    return b


def make_learner(wh, freq=2):
    """Everything from fixed seeds: three modules, a critic of f32 networks mirroring them, targets of
    their own, a bf16 rollout policy, log_alpha = ln 0.5."""
    import torch

    mods = [module(70 + i) for i in range(3)]
    f32 = [wh.policy.MLPPolicy("small", weights=numpy_weights(wh, m), precision="f32") for m in mods]
    targets = [wh.policy.MLPPolicy("small", seed=80 + i, precision="f32") for i in range(2)]
    rollout = wh.policy.MLPPolicy("small", weights=numpy_weights(wh, mods[0]))
    critic = wh.SACCritic(f32[0], f32[1], f32[2], targets[0], targets[1], alpha=1.0, gamma=0.9, n_step=3)
    log_alpha = torch.full((1,), float(np.log(0.5)), device="cuda:0")
    learner = wh.SACLearner(mods[0], mods[1], mods[2], rollout_policy=rollout, critic=critic, log_alpha=log_alpha,
                            target_entropy=TE, lr=1e-2, target_network_update_freq=freq)
    return learner, mods, critic, rollout, targets, log_alpha


def test_one_update_taken_apart(wh, batch):
    import torch

    learner, mods, critic, rollout, targets, log_alpha = make_learner(wh)
    before = copy.deepcopy(mods)
    la0 = log_alpha.clone()
    t0 = [t.packed.clone() for t in targets]
    out = learner.update(batch)
    y, td, stats = out["y"].clone(), out["td"].clone(), out["stats"].clone()
    used = [g.clone() for g in learner.grads]
    assert len(used) == 19 and tuple(stats.shape) == (6,) and tuple(td.shape) == (M,)
    assert abs(critic.alpha - 0.5) < 1e-6
    obs = batch["obs"].view(M * NA, -1)

    # ---- (i) d(loss)/d(logits) on the pre-update modules' logits against float64 autograd, on the CPU
    trainers = [wh.MLPTrainer(m) for m in before]
    logits = [t.forward(obs).clone() for t in trainers]
    mine = {k: torch.empty((M * NA, 9), device="cuda:0") for k in ("dpi", "dq1", "dq2")}
    mine["stats"] = torch.empty(6, device="cuda:0")
    got = wh.sac_losses(*logits, y, batch["actions"], log_alpha=la0, target_entropy=TE, n=batch["n"],
                        weights=batch["weights"], out=mine)
    assert all(got[k].data_ptr() == mine[k].data_ptr() for k in mine)
    pi, q1, q2 = (x.detach().cpu().double().requires_grad_() for x in logits)
    n = batch["n"].cpu().numpy()
    live = torch.as_tensor((np.arange(NA)[None, :] < np.clip(n, 0, NA)[:, None]).reshape(-1))
    w = batch["weights"].cpu().double().repeat_interleave(NA)
    a = batch["actions"].cpu().long().reshape(-1)
    a = torch.where((a >= 0) & (a < 9), a, torch.full_like(a, 4))
    yy = y.cpu().double().reshape(-1)
    alpha, scale = float(np.exp(np.float64(la0.item()))), 1.0 / (M * NA)
    logp = torch.log_softmax(pi, dim=1)
    qm = torch.minimum(q1, q2).detach()
    actor = scale * ((logp.exp() * (alpha * logp - qm)).sum(dim=1) * live).sum()
    r = torch.arange(M * NA)
    c1 = scale * (0.5 * w * (q1[r, a] - yy) ** 2 * live).sum()
    c2 = scale * (0.5 * w * (q2[r, a] - yy) ** 2 * live).sum()
    T = scale * ((logp.exp() * (logp + TE)).sum(dim=1) * live).sum().detach()
    (actor + c1 + c2).backward()
    L = float(pi.detach().abs().max())
    Qm = float(max(q1.detach().abs().max(), q2.detach().abs().max()))
    b = lc.bounds(M, NA, alpha=alpha, log_alpha=float(la0.item()), target_entropy=TE, scale=scale, L=L, Qm=Qm,
                  Ym=float(yy.abs().max()))
    for k, ref in (("dpi", pi.grad), ("dq1", q1.grad), ("dq2", q2.grad)):
        err = float((mine[k].cpu().double() - ref).abs().max())
        print(k, "error / bound", err / (b["dpi"] if k == "dpi" else b["dq"]))
        assert err <= (b["dpi"] if k == "dpi" else b["dq"]), (k, err)
        assert not mine[k].view(M, NA, 9)[6].any(), "the n = -1 sample contributes exact zeros"
    c1, c2, actor = c1.item(), c2.item(), actor.item()
    want = [c1, c2, actor, -float(la0.item()) * float(T), -float(T), float(live.sum())]
    for j, k in enumerate(lc.STAT_KEYS[:5]):
        assert abs(float(mine["stats"][j]) - want[j]) <= b[k] + 1e-7 * abs(want[j]), k
    assert float(mine["stats"][5]) == want[5] == (M - 1) * NA
    assert torch.equal(mine["stats"], stats), "the learner's stats are sac_losses' on its logits"

    # ---- (ii) the gradients the learner used are MLPTrainer.backward of those dlogits, bit for bit
    ref_grads = []
    for t, k in zip(trainers, ("dpi", "dq1", "dq2")):
        g = t.backward(mine[k])
        ref_grads += [g[kk].clone() for kk in KEYS]
    ref_grads.append(mine["stats"][4:5])
    for i, (x, z) in enumerate(zip(used, ref_grads)):
        assert torch.equal(x, z), f"gradient {i}"

    # ---- (iii) every parameter and log_alpha: one wh_adam_step by hand on the saved state and gradients
    hand = [wh.policy.weights_of(m)[k] for m in before for k in KEYS] + [la0]
    wh.DeviceAdam(hand, lr=1e-2).step(ref_grads)
    now = [wh.policy.weights_of(m)[k] for m in mods for k in KEYS] + [log_alpha]
    for i, (x, z) in enumerate(zip(now, hand)):
        assert torch.equal(x, z), f"parameter {i}"
    assert not torch.equal(log_alpha, torch.full_like(log_alpha, float(np.log(0.5))))
    # (Adam's first step moves every element with a gradient by lr: the sign of stats[4] decides log_alpha's)
    assert abs(abs(float(log_alpha.item()) - float(np.log(0.5))) - 1e-2) < 1e-5

    # ---- (iv) the blobs are the new parameters' packing
    for net, m, prec in ((rollout, mods[0], "bf16"), (critic.policy, mods[0], "f32"), (critic.q1, mods[1], "f32"),
                         (critic.q2, mods[2], "f32")):
        fresh = wh.policy.MLPPolicy("small", weights=numpy_weights(wh, m), precision=prec)
        assert torch.equal(net.packed, fresh.packed)

    # ---- (v) targets: untouched after one update, the Q networks' blobs after the second
    assert torch.equal(targets[0].packed, t0[0]) and torch.equal(targets[1].packed, t0[1])
    learner.update(batch)
    assert torch.equal(targets[0].packed, critic.q1.packed) and torch.equal(targets[1].packed, critic.q2.packed)
    assert not torch.equal(targets[0].packed, t0[0])


def test_an_update_on_a_side_stream_gives_the_default_streams_bytes(wh, batch):
    import torch

    def state(parts):
        learner, mods, critic, rollout, targets, log_alpha = parts
        ts = [wh.policy.weights_of(m)[k] for m in mods for k in KEYS] + [log_alpha] + learner.adam.m + learner.adam.v
        ts += [n.packed for n in (rollout, critic.policy, critic.q1, critic.q2, *targets)]
        return [t.clone() for t in ts]

    a, b = make_learner(wh, freq=2), make_learner(wh, freq=2)
    oa = a[0].update(batch)
    ob = b[0].update(batch)
    assert all(torch.equal(oa[k], ob[k]) for k in oa)
    oa = {k: v.clone() for k, v in a[0].update(batch).items()}
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ob = {k: v.clone() for k, v in b[0].update(batch).items()}
    side.synchronize()
    torch.cuda.synchronize()
    for k in oa:
        assert torch.equal(oa[k], ob[k]), k
    for i, (x, z) in enumerate(zip(state(a), state(b))):
        assert torch.equal(x, z), f"tensor {i}"


def test_device_adam_checkpoint_round_trip(wh):
    import torch

    torch.manual_seed(3)
    p = [torch.randn(300, device="cuda:0"), torch.randn(7, 5, device="cuda:0")]
    q = [t.clone() for t in p]
    grads = [[torch.randn_like(t) for t in p] for _ in range(3)]
    a = wh.DeviceAdam(p)
    a.step(grads[0])
    a.step(grads[1])
    saved, p_at_2 = a.state_dict(), [t.clone() for t in p]
    a.step(grads[2])
    b = wh.DeviceAdam(q)
    b.load_state_dict(saved)
    for t, s in zip(q, p_at_2):
        t.copy_(s)
    b.step(grads[2])
    assert b.t == 3 and all(torch.equal(x, z) for x, z in zip(p, q))
    with pytest.raises(ValueError):
        a.step(grads[0][:1])
    with pytest.raises(ValueError):
        a.step([grads[0][0], torch.zeros(7, 6, device="cuda:0")])
