"""The multi-network training entry points (wh_mlp_train_forward_multi / wh_mlp_backward_multi,
csrc/mlp_train.h) on the device:

  * exact against float64, not against the code under test: on the integer-valued networks of
    tests/mlp_train_multi_cases.py (the condition is held by tests/test_mlp_train_multi_cpu.py) every
    job's h0, h1, logits and six gradients are np.array_equal to its own network's float64 reference, for
    three networks at every shape (and four at two of them), outputs and `work` pre-filled with NaN, a
    64-byte 0xA5 guard behind every output and every `work`;
  * bit-equal to the single-network entry points on real-valued weights, for 1 .. 4 networks, jobs 0 and 1
    reading one obs pointer, also from a side stream and on a second call after re-poisoning;
  * rows == 0 gives zero gradients for every job, nnets == 0 writes nothing;
  * warehouse.train_forward_many / train_backward_many return each trainer's own buffers with the bytes of
    the trainers' single calls, and a single trainer.backward after a many-forward agrees;
  * SACLearner(fused_train=True) and (fused_train=False) leave byte-equal parameters, Adam moments, blobs,
    stats, td and y after two updates."""
import copy
import ctypes

import numpy as np
import pytest

import mlp_exact_cases as mx
import mlp_train_multi_cases as mm

pytestmark = pytest.mark.gpu

GRADS = ("w0", "b0", "w1", "b1", "w2", "b2")
ACTS = ("h0", "h1", "logits")
GUARD = 64


@pytest.fixture(scope="module")
def wh():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    import warehouse
    import warehouse.policy  # noqa: F401
    import warehouse.train  # noqa: F401

    return warehouse


class Native:
    """Several networks of one shape and one batch size on the device with guarded outputs, driven
    through the C ABI itself: all of them in one multi call, or one of them in the single calls."""

    def __init__(self, variant, rows, cases, share_obs=()):
        """cases: per job (w, x, dz).  share_obs: pairs (i, j): job i reads job j's obs buffer."""
        import torch
        from warehouse import _native as nat

        self.torch, self.nat = torch, nat
        self.dev = torch.device("cuda", torch.cuda.current_device())
        in_dim, H0, H1 = mx.VARIANT_DIMS[variant]
        self.rows, self.n = rows, len(cases)
        self.desc = nat.WhMlpDesc(in_dim, H0, H1, 9, nat.WH_MLP_F32)
        nbytes = ctypes.c_int64()
        nat.check(nat.lib().wh_mlp_train_query(ctypes.byref(self.desc), rows, ctypes.byref(nbytes)), "query")
        self.shapes = dict(h0=(rows, H0), h1=(rows, H1), logits=(rows, 9), w0=(H0, in_dim), b0=(H0,), w1=(H1, H0),
                           b1=(H1,), w2=(9, H1), b2=(9,))
        self.w, self.x, self.dz, self.out, self.work = [], [], [], [], []
        for w, x, d in cases:
            self.w.append({k: self._up(w[k]) for k in GRADS})
            self.x.append(self._up(x, pad=True))
            self.dz.append(self._up(d, pad=True))
            self.out.append({k: self._guarded(4 * int(np.prod(s))) for k, s in self.shapes.items()})
            self.work.append(self._guarded(int(nbytes.value)))
        for i, j in share_obs:
            assert np.array_equal(cases[i][1], cases[j][1])
            self.x[i] = self.x[j]
        self.jobs = (nat.WhMlpTrainJob * max(1, self.n))(*[self._job(i) for i in range(self.n)])

    def _up(self, a, pad=False):
        # (a copy: the cases are read-only; an empty array gets an address of its own)
        t = self.torch.as_tensor(np.array(a, np.float32)).to(self.dev).contiguous()
        return t if t.numel() or not pad else self.torch.zeros(16, device=self.dev)

    def _guarded(self, nbytes):
        t = self.torch.empty(nbytes + GUARD, dtype=self.torch.uint8, device=self.dev)
        t[nbytes:] = 0xA5
        return t

    def _job(self, i):
        nat, o = self.nat, self.out[i]
        return nat.WhMlpTrainJob(nat.WhMlpWeights(*[self.w[i][k].data_ptr() for k in GRADS]), self.x[i].data_ptr(),
                                 o["h0"].data_ptr(), o["h1"].data_ptr(), o["logits"].data_ptr(), self.dz[i].data_ptr(),
                                 nat.WhMlpGrads(*[o[k].data_ptr() for k in GRADS]), self.work[i].data_ptr())

    def poison(self, keys=ACTS + GRADS + ("work",)):
        for i in range(self.n):
            for k in keys:
                t = self.work[i] if k == "work" else self.out[i][k]
                t[:t.numel() - GUARD].view(self.torch.float32).fill_(float("nan"))

    def forward_multi(self, stream=0, nnets=None):
        nat = self.nat
        nat.check(nat.lib().wh_mlp_train_forward_multi(ctypes.byref(self.desc), self.n if nnets is None else nnets,
                                                       self.jobs, self.rows, stream), "wh_mlp_train_forward_multi")

    def backward_multi(self, stream=0, nnets=None):
        nat = self.nat
        nat.check(nat.lib().wh_mlp_backward_multi(ctypes.byref(self.desc), self.n if nnets is None else nnets,
                                                  self.jobs, self.rows, stream), "wh_mlp_backward_multi")

    def forward_single(self, i):
        nat, j = self.nat, self.jobs[i]
        nat.check(nat.lib().wh_mlp_train_forward(ctypes.byref(self.desc), ctypes.byref(j.w), self.rows, j.obs, j.h0, j.h1,
                                                 j.logits, 0), "wh_mlp_train_forward")

    def backward_single(self, i):
        nat, j = self.nat, self.jobs[i]
        nat.check(nat.lib().wh_mlp_backward(ctypes.byref(self.desc), ctypes.byref(j.w), self.rows, j.obs, j.h0, j.h1,
                                            j.dlogits, ctypes.byref(j.g), j.work, 0), "wh_mlp_backward")

    def get(self, i, k):
        t = self.out[i][k]
        return t[:t.numel() - GUARD].view(self.torch.float32).cpu().numpy().reshape(self.shapes[k])

    def raw(self, keys=ACTS + GRADS):
        """Every output of every job, guard included, as bytes."""
        return {(i, k): self.out[i][k].cpu().numpy().tobytes() for i in range(self.n) for k in keys}

    def guards_intact(self):
        ts = [t for o in self.out for t in o.values()] + self.work
        return all(bool((t[t.numel() - GUARD:] == 0xA5).all()) for t in ts)


def assert_equal(what, got, want):
    got = got.astype(np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert not np.isnan(got).any(), f"{what}: NaN"
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} values differ, first at {i}: kernel {got[i]!r}, "
                             f"reference {want[i]!r}; largest |d| {np.abs(got - want).max()!r}")


def exact(variant, rows, nnets):
    cases = [mm.job(variant, rows, k) for k in range(nnets)]
    n = Native(variant, rows, [c[:3] for c in cases])
    n.poison()
    n.forward_multi()
    n.backward_multi()
    for i, (w, x, d, fwd, ref) in enumerate(cases):
        what = f"{variant} rows {rows} job {i} of {nnets}"
        for k in ACTS:
            assert_equal(f"{what} {k}", n.get(i, k), fwd[k])
        for k in GRADS:
            assert_equal(f"{what} g{k}", n.get(i, k), ref[k])
    assert n.guards_intact(), f"{variant} rows {rows}: a guard behind an output or a work buffer changed"


@pytest.mark.parametrize("variant,rows", mm.SHAPES, ids=lambda v: str(v))
def test_three_integer_networks_are_exact(wh, variant, rows):
    exact(variant, rows, 3)


@pytest.mark.parametrize("variant,rows", [("small", 33), ("medium", 513)], ids=lambda v: str(v))
def test_four_integer_networks_are_exact(wh, variant, rows):
    exact(variant, rows, 4)


@pytest.mark.parametrize("nnets", (1, 2, 3, 4))
@pytest.mark.parametrize("variant,rows", mm.REAL_SHAPES, ids=lambda v: str(v))
def test_bit_equal_to_the_single_network_entry_points(wh, variant, rows, nnets):
    import torch

    cases = [mm.real_job(variant, rows, k) for k in range(nnets)]
    n = Native(variant, rows, cases, share_obs=((1, 0),) if nnets > 1 else ())
    if nnets > 1:
        assert n.jobs[0].obs == n.jobs[1].obs and all(n.jobs[i].obs != n.jobs[0].obs for i in range(2, nnets))
    n.poison()
    for i in range(nnets):
        n.forward_single(i)
        n.backward_single(i)
    want = n.raw()
    assert not any(np.isnan(np.frombuffer(v[:-GUARD], np.float32)).any() for v in want.values())
    # the three networks' answers differ: a job routed to another network's pointers would show
    assert len({want[(i, "logits")] for i in range(nnets)}) == nnets
    assert len({want[(i, "w0")] for i in range(nnets)}) == nnets

    def run(stream=0):
        n.poison()
        torch.cuda.synchronize()
        n.forward_multi(stream)
        n.backward_multi(stream)
        torch.cuda.synchronize()
        return n.raw()

    side = torch.cuda.Stream()
    for what, got in (("multi", run()), ("a second call after re-poisoning", run()),
                      ("a side stream", run(side.cuda_stream))):
        for key in want:
            assert got[key] == want[key], (variant, rows, nnets, what, key)
    assert n.guards_intact()


@pytest.mark.parametrize("variant", mx.VARIANTS)
def test_no_rows_give_zero_gradients_and_no_networks_write_nothing(wh, variant):
    import torch

    in_dim = mx.VARIANT_DIMS[variant][0]
    cases = [(mx.network(variant, s), np.zeros((0, in_dim), np.float32), np.zeros((0, 9), np.float32)) for s in mm.SEEDS]
    n = Native(variant, 0, cases)
    n.poison(GRADS + ("work",))
    n.forward_multi()                         # launches nothing
    n.backward_multi()
    torch.cuda.synchronize()
    for i in range(3):
        for k in GRADS:
            g = n.get(i, k)
            assert not np.isnan(g).any() and not g.any(), (variant, i, k)
    assert n.guards_intact()
    # no networks: nothing is written, with rows or without
    for rows in (0, 33):
        cases = [mm.job(variant, 33, k)[:3] for k in range(3)] if rows else cases
        n = Native(variant, rows, cases)
        n.poison()
        n.forward_multi(nnets=0)
        n.backward_multi(nnets=0)
        torch.cuda.synchronize()
        for i in range(3):
            for k in (ACTS if rows else ()) + GRADS:
                assert np.isnan(n.get(i, k)).all(), (variant, rows, i, k)
        assert n.guards_intact()


def make_module(torch, variant, w, dev):
    in_dim, H0, H1 = mx.VARIANT_DIMS[variant]
    L = torch.nn.Linear
    m = torch.nn.Sequential(L(in_dim, H0), torch.nn.ReLU(), L(H0, H1), torch.nn.ReLU(), L(H1, 9)).to(dev)
    with torch.no_grad():
        for i, lin in enumerate(m[j] for j in (0, 2, 4)):
            lin.weight.copy_(torch.as_tensor(np.array(w[f"w{i}"])))
            lin.bias.copy_(torch.as_tensor(np.array(w[f"b{i}"])))
    return m


@pytest.mark.parametrize("variant,rows,shared", [("medium", 513, True), ("small", 1025, False), ("large", 33, True)])
def test_python_surface_returns_each_trainers_own_buffers(wh, variant, rows, shared):
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    cases = [mm.real_job(variant, rows, k) for k in range(3)]
    mods = [make_module(torch, variant, c[0], dev) for c in cases]
    up = lambda a: torch.as_tensor(np.array(a)).to(dev)   # noqa: E731
    obs = [up(cases[0][1])] * 3 if shared else [up(c[1]) for c in cases]
    dz = [up(c[2]) for c in cases]
    # the single calls, on trainers of their own
    single = [wh.MLPTrainer(m) for m in mods]
    want_l = [t.forward(o).clone() for t, o in zip(single, obs)]
    want_a = [[a.clone() for a in t.activations()] for t in single]
    want_g = [{k: v.clone() for k, v in t.backward(d).items()} for t, d in zip(single, dz)]
    many = [wh.MLPTrainer(m) for m in mods]
    got_l = wh.train_forward_many(many, obs[0] if shared else obs)
    assert len(got_l) == 3
    for i, t in enumerate(many):
        assert got_l[i].data_ptr() == t._own("logits", (rows, 9)).data_ptr(), "the trainer's own logits buffer"
        assert torch.equal(got_l[i], want_l[i]), i
        for a, b in zip(t.activations(), want_a[i]):
            assert torch.equal(a, b), i
    # a single backward after the many-forward works, and agrees
    one = {k: v.clone() for k, v in many[1].backward(dz[1]).items()}
    for k in GRADS:
        assert torch.equal(one[k], want_g[1][k]), k
        many[1]._own("g" + k, one[k].shape).fill_(float("nan"))
    got_g = wh.train_backward_many(many, dz)
    assert len(got_g) == 3
    for i, t in enumerate(many):
        for k in GRADS:
            assert got_g[i][k].data_ptr() == t._own("g" + k, got_g[i][k].shape).data_ptr(), "the trainer's own gradient"
            assert torch.equal(got_g[i][k], want_g[i][k]), (i, k)
    # the caller's tensors through `out`, for some trainers only
    mine = {k: torch.full_like(v, float("nan")) for k, v in want_g[2].items()}
    again = wh.train_backward_many(many, dz, out=[None, None, mine])
    assert all(again[2][k] is mine[k] and torch.equal(mine[k], want_g[2][k]) for k in GRADS)
    assert all(torch.equal(again[0][k], want_g[0][k]) for k in GRADS)
    # no rows: empty logits, zero gradients
    empty = torch.empty((0, mx.VARIANT_DIMS[variant][0]), device=dev)
    assert [tuple(x.shape) for x in wh.train_forward_many(many, empty)] == [(0, 9)] * 3
    zero = wh.train_backward_many(many, [torch.empty((0, 9), device=dev)] * 3)
    assert all(not zero[i][k].any() and not torch.isnan(zero[i][k]).any() for i in range(3) for k in GRADS)


# ---------------------------------------------------------------------------------------------- the learner
# tests/test_gpu_learner.py's setup: Small-4, M = 16, a wrapped prioritized ring
KEYS = GRADS
M, NA = 16, 4


def module(seed):
    import torch

    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(37, 256), torch.nn.ReLU(), torch.nn.Linear(256, 256), torch.nn.ReLU(),
                               torch.nn.Linear(256, 9)).to("cuda:0")


def numpy_weights(wh, mod):
    return {k: v.cpu().numpy() for k, v in wh.policy.weights_of(mod).items()}


@pytest.fixture(scope="module")
def batch(wh):
    import torch
    from replay_cases import place_near_end

    env = wh.BatchedWarehouse("small", 8, NA, seed=11, device="cuda:0")
    place_near_end(env)
    buf = wh.ReplayBuffer(env, capacity=4, prioritized=True)
    for _ in range(6):
        buf.step(env.policy("greedy", 0.3))
    rng = np.random.default_rng(5)
    idx = rng.integers(0, len(buf), M)
    idx[3] = idx[9]
    idx[6] = len(buf) + 7                                     # outside the ring: n = -1
    b = {k: v.clone() for k, v in buf.sample(M, idx=idx, rows=True).items()}
    b["weights"] = torch.as_tensor(rng.choice(np.array([0.25, 0.5, 0.75, 1.0], np.float32), M)).to("cuda:0")
    torch.cuda.synchronize()
    return b


def make_learner(wh, mods, fused_train, twin=True):
    import torch

    mods = mods if twin else mods[:2]
    f32 = [wh.policy.MLPPolicy("small", weights=numpy_weights(wh, m), precision="f32") for m in mods]
    targets = [wh.policy.MLPPolicy("small", seed=80 + i, precision="f32") for i in range(len(mods) - 1)]
    rollout = wh.policy.MLPPolicy("small", weights=numpy_weights(wh, mods[0]))
    if twin:
        critic = wh.SACCritic(f32[0], f32[1], f32[2], targets[0], targets[1], alpha=1.0, gamma=0.9, n_step=3)
    else:
        critic = wh.SACCritic(f32[0], f32[1], None, targets[0], None, alpha=1.0, gamma=0.9, n_step=3)
    log_alpha = torch.full((1,), float(np.log(0.5)), device="cuda:0")
    learner = wh.SACLearner(mods[0], mods[1], mods[2] if twin else None, rollout_policy=rollout, critic=critic,
                            log_alpha=log_alpha, target_entropy=0.935, lr=1e-2, target_network_update_freq=2,
                            fused_train=fused_train)
    return learner, mods, critic, rollout, targets, log_alpha


def state(wh, parts):
    learner, mods, critic, rollout, targets, log_alpha = parts
    ts = [wh.policy.weights_of(m)[k] for m in mods for k in KEYS] + [log_alpha] + learner.adam.m + learner.adam.v
    ts += [n.packed for n in (rollout, critic.policy, critic.q1, critic.q2, *targets) if n is not None]
    return [t.clone() for t in ts]


@pytest.mark.parametrize("twin", [True, False], ids=["twin", "no twin"])
def test_fused_and_sequential_learners_leave_the_same_bytes(wh, batch, twin):
    import torch

    mods = [module(70 + i) for i in range(3)]
    a = make_learner(wh, copy.deepcopy(mods), True, twin)
    b = make_learner(wh, copy.deepcopy(mods), False, twin)
    assert a[0].fused_train is True and b[0].fused_train is False
    assert len(a[0].trainers) == (3 if twin else 2)
    start = state(wh, a)
    for step in range(2):
        oa = {k: v.clone() for k, v in a[0].update(batch).items()}
        ob = {k: v.clone() for k, v in b[0].update(batch).items()}
        assert sorted(oa) == ["stats", "td", "y"]
        for k in oa:
            assert oa[k].cpu().numpy().tobytes() == ob[k].cpu().numpy().tobytes(), (step, k)
        assert a[0].last_fused_train is True and b[0].last_fused_train is False
    sa, sb = state(wh, a), state(wh, b)
    assert len(sa) == len(sb)
    for i, (x, z) in enumerate(zip(sa, sb)):
        assert x.cpu().numpy().tobytes() == z.cpu().numpy().tobytes(), f"tensor {i}"
    assert not all(torch.equal(x, z) for x, z in zip(sa[:18], start[:18])), "the updates moved the parameters"
    # the default is one of the two routes, and computes the same
    c = make_learner(wh, copy.deepcopy(mods), None, twin)
    assert c[0].fused_train is None and c[0].use_fused_train(M * NA) in (True, False)
    for step in range(2):
        c[0].update(batch)
    assert c[0].last_fused_train == c[0].use_fused_train(M * NA)
    for i, (x, z) in enumerate(zip(state(wh, c), sa)):
        assert torch.equal(x, z), f"default route, tensor {i}"
