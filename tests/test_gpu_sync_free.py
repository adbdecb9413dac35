"""The sync-free learner update on the GPU: wh_adam_step_clock and wh_sac_td_la against the host engine and
the float64 model (the bodies of tests/sync_free_cases.py), SACLearner(sync_free=True) against the default
route on the first update, a captured update replayed against the same updates made eagerly, capture()
leaving the learner as it found it, and the host syncs of the two routes under torch's sync debug mode.

The learners are Small-4 and Medium-8 at M = 64 (256 rows: the one-workgroup loss; 512 rows: the two-launch
loss), f32 master modules, five bf16 critic networks reading the fragment operand, a prioritized ring of
B = 16 envs and 8 slots, log_alpha = 0 (alpha exactly 1 on both routes), target_network_update_freq = 2.

Largest errors of device wh_sac_td_la seen at the three log_alphas, as fractions of the widened bounds (y,
td_rows, td): 0.055, 0.045, 0.0091."""
import numpy as np
import pytest

import sync_free_cases as sf

pytestmark = pytest.mark.gpu

KEYS = ("w0", "b0", "w1", "b1", "w2", "b2")
CONFIGS = (("small", 4), ("medium", 8))
M = 64


@pytest.fixture(scope="module")
def wh():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    import warehouse
    import warehouse.policy  # noqa: F401

    return warehouse


@pytest.fixture(scope="module")
def nat():
    from warehouse import _native

    return _native


# ----------------------------------------------------------------------------- the entry points
def test_engines_agree_on_the_clock_and_the_tensors(nat):
    sf.case_engines_agree_on_the_clock(nat, steps=20)


def test_step_clock_on_the_device_is_adam_step_with_the_clocks_table(nat):
    sf.case_step_is_adam_step_with_the_clocks_table(nat, nat.lib(), "cuda:0", 999)


@pytest.mark.parametrize("Ms", sf.TD_MS)
@pytest.mark.parametrize("NA", sf.TD_NAS)
def test_td_la_on_the_device(nat, NA, Ms):
    print("device NA", NA, "M", Ms, "errors / bounds", sf.case_td_la(nat, nat.lib(), "cuda:0", NA, Ms))


def test_device_adam_checkpoints_carry_the_clock(wh, nat):
    """A state saved from a device clock after three steps loads into a fresh device-step optimiser (t and
    both products as saved) and into a host-count one (which ignores the products); a state of the
    host-count form loads into a device-step optimiser with the products rebuilt by t multiplications,
    which are the tick's.  The fourth step gives the same tensors bit for bit on the two device clocks; the
    host-count optimiser's table is pow's, within one f32 ulp of the clock's, so its tensors are not
    compared bit for bit."""
    import torch

    torch.manual_seed(3)
    p0 = [torch.randn(300, device="cuda:0"), torch.randn(7, 5, device="cuda:0")]
    grads = [[torch.randn_like(t) for t in p0] for _ in range(4)]

    def fresh(**kw):
        return wh.DeviceAdam([t.clone() for t in p0], lr=1e-3, **kw)

    def products(adam):
        c = adam._read_clock()
        return int(c.t), float(c.beta1_t), float(c.beta2_t)

    a = fresh(device_step=True)
    assert a.t == 0 and products(a) == (0, 1.0, 1.0)
    for g in grads[:3]:
        a.step(g)
    saved, p_at_3 = a.state_dict(), [t.clone() for t in a.tensors]
    want = nat.adam_clock(3, *a.betas)
    assert saved["step"] == 3 and saved["beta_t"] == (want.beta1_t, want.beta2_t) == products(a)[1:]
    a.step(grads[3])

    b = fresh(device_step=True)                               # device clock <- device clock
    b.load_state_dict(saved)
    assert b.t == 3 and products(b) == (3,) + saved["beta_t"]
    c = fresh(device_step=True)                               # device clock <- host-count form: products rebuilt
    c.load_state_dict({k: v for k, v in saved.items() if k != "beta_t"})
    assert products(c) == products(b)
    h = fresh()                                               # host count <- device clock
    h.load_state_dict(saved)
    assert h.t == 3 and h.clock is None and "beta_t" not in h.state_dict()
    for o in (b, c, h):
        for t, s in zip(o.tensors, p_at_3):
            t.copy_(s)
        assert all(torch.equal(x, y) for x, y in zip(o.m + o.v, saved["m"] + saved["v"]))
        o.step(grads[3])
    assert a.t == b.t == c.t == h.t == 4 and products(a) == products(b) == products(c)
    for o in (b, c):
        assert all(torch.equal(x, y) for x, y in zip(o.tensors + o.m + o.v, a.tensors + a.m + a.v))
    assert all(torch.equal(x, y) for x, y in zip(h.m + h.v, a.m + a.v))       # m and v do not see the bias corrections
    # p: two table fields one f32 ulp apart move the step (at most a few lr = 1e-3) by under 4 ulps of it, 5e-10,
    # which can move the rounding of p - step by one ulp of p (1.2e-7 relative)
    assert all(torch.allclose(x, y, rtol=2.5e-7, atol=1e-9) for x, y in zip(h.tensors, a.tensors))
    a.t = 10                                                  # the setter rebuilds the clock as the tick would
    w = nat.adam_clock(10, *a.betas)
    assert products(a) == (10, w.beta1_t, w.beta2_t)


# ----------------------------------------------------------------------------- the learner
def make(wh, variant, na, sync_free, freq=2):
    """One learner and its ring, everything from fixed seeds: every call gives a bit-identical copy."""
    import torch
    from warehouse._geometry import GEOMETRY
    from warehouse.policy import HIDDEN, MLPPolicy, weights_of

    dev = torch.device("cuda", 0)
    in_dim, (h0, h1) = 9 * GEOMETRY[variant]["R"] + 1, HIDDEN[variant]
    mods = []
    for i in range(3):
        torch.manual_seed(40 + i)
        mods.append(torch.nn.Sequential(torch.nn.Linear(in_dim, h0), torch.nn.ReLU(), torch.nn.Linear(h0, h1),
                                        torch.nn.ReLU(), torch.nn.Linear(h1, 9)).to(dev))
    nets = [MLPPolicy(variant, seed=50 + i) for i in range(5)]
    for net, m in zip(nets[:3], mods):
        net.load_weights(weights_of(m))
    critic = wh.SACCritic(nets[0], nets[1], nets[2], nets[3], nets[4], alpha=1.0, gamma=0.99)
    learner = wh.SACLearner(*mods, rollout_policy=nets[0], critic=critic, log_alpha=torch.zeros(1, device=dev),
                            lr=1e-3, target_network_update_freq=freq, sync_free=sync_free)
    env = wh.BatchedWarehouse(variant, 16, na, seed=3, device=dev)
    env.reset()
    buf = wh.ReplayBuffer(env, capacity=8, prioritized=True)
    for _ in range(10):
        buf.step(env.policy("greedy", 0.2))
    return learner, buf


def state(learner, buf=None):
    """Clones of everything an update writes (and the ring's tree), by name."""
    c = learner.critic
    s = {f"param {i}": t for i, t in enumerate(learner.adam.tensors)}          # the 18 tensors and log_alpha
    s.update({f"m {i}": t for i, t in enumerate(learner.adam.m)})
    s.update({f"v {i}": t for i, t in enumerate(learner.adam.v)})
    s.update(rollout=learner.rollout_policy.packed, q1=c.q1.packed, q2=c.q2.packed, q1_target=c.q1_target.packed,
             q2_target=c.q2_target.packed, log_alpha=learner.log_alpha)
    if buf is not None:
        s.update(leaf=buf.prio_leaf, node=buf.prio_node, max_q=buf.prio_max_q)
    return {k: v.clone() for k, v in s.items()}


def results(learner, out):
    r = {k: v.clone() for k, v in out.items()}
    r.update({f"grad {i}": g.clone() for i, g in enumerate(learner.grads)})
    return r


def same(a, b, what):
    import torch

    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs"


@pytest.mark.parametrize("variant,na", CONFIGS)
def test_sync_free_and_default_routes_agree_on_the_first_update(wh, variant, na):
    (a, bufa), (b, bufb) = make(wh, variant, na, False), make(wh, variant, na, True)
    same(state(a, bufa), state(b, bufb), "before")
    batch = {k: v.clone() for k, v in bufa.sample(M, draw=7, rows=True, fragments=True).items()}
    ra = results(a, a.update(batch))
    rb = results(b, b.update(batch))
    assert len(ra) == 3 + 19 and tuple(ra["y"].shape) == (M, na)
    same(ra, rb, "update 1")
    same(state(a), state(b), "after update 1")
    assert a.adam.t == b.adam.t == 1 and b.adam.clock is not None and a.adam.clock is None
    assert float(a.log_alpha) != 0.0                        # the update moved what the routes read differently


@pytest.mark.parametrize("variant,na", CONFIGS)
def test_replay_equals_eager(wh, variant, na):
    import torch

    (e, bufe), (g, bufg) = make(wh, variant, na, True), make(wh, variant, na, True)
    first = bufg.sample(M, draw=99, rows=True, fragments=True)
    before = state(g, bufg)
    graph = g.capture(first, buf=bufg)
    same(before, state(g, bufg), "capture() left the learner")
    assert g.updates == 0 and g.adam.t == 0
    with pytest.raises(ValueError):
        graph.replay({k: v.clone() for k, v in first.items()})
    for k in range(5):
        be = bufe.sample(M, draw=200 + k, rows=True, fragments=True)
        re = results(e, e.update(be))
        bufe.update_priorities(be["idx_out"], re["td"])
        bg = bufg.sample(M, draw=200 + k, rows=True, fragments=True)
        assert all(torch.equal(be[x], bg[x]) for x in be), f"update {k + 1}: the two rings drew different batches"
        out = graph.replay(bg)
        assert out is graph.out and g.updates == k + 1
        same(re, results(g, out), f"update {k + 1}")
        same(state(e, bufe), state(g, bufg), f"after update {k + 1}")
        synced = torch.equal(g.critic.q1_target.packed, g.critic.q1.packed) and \
            torch.equal(g.critic.q2_target.packed, g.critic.q2.packed)
        assert synced == ((k + 1) % 2 == 0), f"targets after update {k + 1}"
    assert g.adam.t == 5 and e.adam.t == 5
    assert bool(torch.isfinite(out["stats"]).all()) and float(out["stats"][5]) > 0


def test_capture_leaves_the_learner_untouched(wh):
    """Without a ring, at an update count where the warm-up runs a target sync (freq = 1)."""
    g, buf = make(wh, "small", 4, True, freq=1)
    batch = {k: v.clone() for k, v in buf.sample(M, draw=3, rows=True, fragments=True, uniform=True).items()}
    g.update(batch)
    before, updates, host = state(g, buf), g.updates, [n.weights for n in (g.critic.q1_target, g.rollout_policy)]
    graph = g.capture(batch)
    same(before, state(g, buf), "capture()")
    assert g.updates == updates == 1 and g.adam.t == 1
    assert [n.weights for n in (g.critic.q1_target, g.rollout_policy)] == host
    graph.replay()
    assert g.updates == 2 and g.adam.t == 2
    with pytest.raises(ValueError, match="sync_free"):
        make(wh, "small", 4, False)[0].capture(batch)


def test_sync_free_update_makes_no_host_sync_and_the_default_makes_one(wh):
    import torch

    (a, buf), (b, _) = make(wh, "small", 4, False), make(wh, "small", 4, True)
    batch = {k: v.clone() for k, v in buf.sample(M, draw=5, rows=True, fragments=True).items()}
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        b.update(batch)
        b.update(batch)
        with pytest.raises(RuntimeError, match="synchroniz"):
            a.update(batch)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    assert b.updates == 2 and b.adam.t == 2 and a.updates == 0
