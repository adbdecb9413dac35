"""The MLP training kernels (wh_mlp_train_forward / wh_mlp_backward, csrc/mlp_train.h) on the device,
against the float64 reference of tests/mlp_grad_cases.py (the conditions that make the comparisons mean
something are held by tests/test_mlp_grad_cpu.py):

  * tolerance 0 on the integer-valued networks: h0, h1, logits and the six gradients are np.array_equal
    to float64, at 1 / 31 / 33 / 257 / 300 rows of every variant, 513 rows of Medium (the 32-row tile
    edge, many row blocks and a ragged last one, and above 512 rows the weight gradients in two K slices
    with their second pass) and 1,024 / 1,025 rows of Small (the last row count on the 32 x 32 tile
    geometry and the first on the 64 x 64 one, two and three slices), gradients and `work` pre-filled
    with NaN, a 64-byte 0xA5 guard behind every output;
  * bit-equal repeats on the real-valued network, also from another stream;
  * the real-valued network within error_bound (derived, for any summation order), the backward reference
    taking the kernel's own h > 0 masks, which may differ from float64's only where |pre| lies within the
    forward bound and at no more than 0.2 % of a layer's units;
  * the autograd surface: mlp_logits fills param.grad, accumulates, agrees with torch's autograd of
    module(obs), feeds the device packer after an optimiser step, and takes an empty batch.

Largest error / bound seen per tensor (printed by test_real_valued_network_within_the_bound, run with -s)
are recorded in DESIGN.md §7."""
import ctypes

import numpy as np
import pytest

import mlp_exact_cases as mx
import mlp_grad_cases as mg

pytestmark = pytest.mark.gpu

GRADS = ("w0", "b0", "w1", "b1", "w2", "b2")
GUARD = 64


@pytest.fixture(scope="module")
def wh():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    import warehouse
    import warehouse.train  # noqa: F401

    return warehouse


class Native:
    """One network and batch on the device with guarded outputs, driven through the C ABI itself."""

    def __init__(self, wh, variant, w, x, dz):
        import torch
        from warehouse import _native as nat

        self.torch, self.nat = torch, nat
        self.dev = torch.device("cuda", torch.cuda.current_device())
        in_dim, H0, H1 = mx.VARIANT_DIMS[variant]
        self.rows = rows = x.shape[0]
        self.desc = nat.WhMlpDesc(in_dim, H0, H1, 9, nat.WH_MLP_F32)
        up = lambda a: torch.as_tensor(np.array(a, np.float32)).to(self.dev).contiguous()   # noqa: E731  (a copy: the cases are read-only)
        self.w = {k: up(w[k]) for k in GRADS}
        self.x, self.dz = up(x), up(dz)
        n = ctypes.c_int64()
        nat.check(nat.lib().wh_mlp_train_query(ctypes.byref(self.desc), rows, ctypes.byref(n)), "query")
        self.shapes = dict(h0=(rows, H0), h1=(rows, H1), logits=(rows, 9), **{k: tuple(w[k].shape) for k in GRADS})
        self.out = {k: self._guarded(4 * int(np.prod(s))) for k, s in self.shapes.items()}
        self.work = self._guarded(int(n.value))
        self.ws = nat.WhMlpWeights(*[self.w[k].data_ptr() for k in GRADS])
        self.gs = nat.WhMlpWeights(*[self.out[k].data_ptr() for k in GRADS])

    def _guarded(self, nbytes):
        t = self.torch.empty(nbytes + GUARD, dtype=self.torch.uint8, device=self.dev)
        t[nbytes:] = 0xA5
        return t

    def poison(self, keys):
        for k in keys:
            t = self.work if k == "work" else self.out[k]
            t[:t.numel() - GUARD].view(self.torch.float32).fill_(float("nan"))

    def forward(self, stream=0):
        nat, o = self.nat, self.out
        nat.check(nat.lib().wh_mlp_train_forward(ctypes.byref(self.desc), ctypes.byref(self.ws), self.rows, self.x.data_ptr(),
                                                 o["h0"].data_ptr(), o["h1"].data_ptr(), o["logits"].data_ptr(), stream),
                  "wh_mlp_train_forward")

    def backward(self, stream=0):
        nat, o = self.nat, self.out
        nat.check(nat.lib().wh_mlp_backward(ctypes.byref(self.desc), ctypes.byref(self.ws), self.rows, self.x.data_ptr(),
                                            o["h0"].data_ptr(), o["h1"].data_ptr(), self.dz.data_ptr(), ctypes.byref(self.gs),
                                            self.work.data_ptr(), stream), "wh_mlp_backward")

    def get(self, k):
        t = self.out[k]
        return t[:t.numel() - GUARD].view(self.torch.float32).cpu().numpy().reshape(self.shapes[k])

    def raw(self, keys=GRADS):
        return {k: self.out[k].cpu().numpy().copy() for k in keys}

    def guards_intact(self):
        return all(bool((t[t.numel() - GUARD:] == 0xA5).all()) for t in list(self.out.values()) + [self.work])


def assert_equal(what, got, want):
    got = got.astype(np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert not np.isnan(got).any(), f"{what}: NaN"
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} values differ, first at {i}: kernel {got[i]!r}, "
                             f"reference {want[i]!r}; largest |d| {np.abs(got - want).max()!r}")


@pytest.mark.parametrize("variant,rows", mg.EXACT_CASES, ids=lambda v: str(v))
def test_integer_network_is_exact(wh, variant, rows):
    w, x, d, fwd, ref = mg.exact_case(variant, rows)
    n = Native(wh, variant, w, x, d)
    n.poison(("h0", "h1", "logits", "work") + GRADS)
    n.forward()
    n.backward()
    what = f"{variant} rows {rows}"
    for k in ("h0", "h1", "logits"):
        assert_equal(f"{what} {k}", n.get(k), fwd[k])
    for k in GRADS:
        assert_equal(f"{what} g{k}", n.get(k), ref[k])
    assert n.guards_intact(), f"{what}: a guard behind an output changed"


@pytest.mark.parametrize("rows", (257, 513))
@pytest.mark.parametrize("variant", ("medium", "large"))
def test_repeats_are_bit_equal(wh, variant, rows):
    import torch

    w, x, d, fwd = mg.real_case(variant, rows)
    n = Native(wh, variant, w, x, d)
    n.forward()
    n.backward()
    first = n.raw()
    n.poison(("work",) + GRADS)
    n.backward()
    again = n.raw()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    n.poison(("work",) + GRADS)
    torch.cuda.synchronize()
    n.backward(stream=side.cuda_stream)
    side.synchronize()
    other = n.raw()
    for k in GRADS:
        assert first[k].tobytes() == again[k].tobytes(), (variant, rows, k, "second call")
        assert first[k].tobytes() == other[k].tobytes(), (variant, rows, k, "another stream")
    assert n.guards_intact()


def check_masks(what, got, fwd, E):
    """The kernel's h > 0 masks against float64's: different only inside the band, and rarely."""
    masks = []
    for layer, (h, pre, e) in enumerate(((got["h0"], fwd["pre0"], E["h0"]), (got["h1"], fwd["pre1"], E["h1"]))):
        m = h > 0
        flips = m != (pre > 0)
        print(f"{what}: layer {layer} mask differs from float64's at {int(flips.sum())} of {flips.size} units")
        assert not (flips & (np.abs(pre) > e)).any(), f"{what}: layer {layer} mask differs outside the band"
        assert flips.mean() <= 0.002, f"{what}: layer {layer} mask differs at {flips.mean():.2%} of units"
        masks.append(m)
    return tuple(masks)


@pytest.mark.parametrize("rows", mg.ROWS_REAL)
@pytest.mark.parametrize("variant", ("medium", "large"))
def test_real_valued_network_within_the_bound(wh, variant, rows):
    real_within_the_bound(wh, variant, rows)


def test_eight_row_slices_within_the_bound(wh):
    """4,096 rows of Large: the weight gradients in eight K slices (the other cases reach two), 64 row
    blocks, and the most units of any case near the mask edge."""
    real_within_the_bound(wh, "large", 4096)


def real_within_the_bound(wh, variant, rows):
    w, x, d, fwd = mg.real_case(variant, rows)
    n = Native(wh, variant, w, x, d)
    n.poison(("h0", "h1", "logits", "work") + GRADS)
    n.forward()
    n.backward()
    got = {k: n.get(k).astype(np.float64) for k in ("h0", "h1", "logits") + GRADS}
    what = f"{variant} rows {rows}"
    masks = check_masks(what, got, fwd, mg.forward_bound(w, x, fwd))
    ref = dict(mg.reference_backward(w, x, d, masks=masks, fwd=fwd), h0=fwd["h0"], h1=fwd["h1"], logits=fwd["logits"])
    E = mg.error_bound(w, x, d, masks=masks, fwd=fwd)
    worst = {}
    for k in got:
        assert not np.isnan(got[k]).any(), f"{what} {k}: NaN"
        err = np.abs(got[k] - ref[k])
        ratio = np.where(err > 0, err / np.maximum(E[k], 1e-300), 0.0)
        worst[k] = float(ratio.max())
    print(f"{what}: largest error / bound per tensor:", {k: "%.3f" % v for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= 1.0, f"{what} {k}: error {v:.3f} x the bound"
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


def grads_of(module):
    return {f"{n}{i}": getattr(module[j], a).grad for i, j in enumerate((0, 2, 4)) for n, a in (("w", "weight"), ("b", "bias"))}


def test_autograd_surface(wh):
    import torch

    variant, rows = "medium", 300
    dev = torch.device("cuda", torch.cuda.current_device())
    w, x, _, fwd = mg.real_case(variant, rows)
    c = np.random.default_rng([9, rows]).uniform(-1, 1, (rows, 9)).astype(np.float32)
    module = make_module(torch, variant, w, dev)
    obs, cd = torch.as_tensor(x.copy()).to(dev), torch.as_tensor(c).to(dev)
    # the kernel's masks: the explicit form runs the same forward
    tr = wh.MLPTrainer(module)
    lg = tr.forward(obs)
    Ef = mg.forward_bound(w, x, fwd)
    acts = dict(zip(("h0", "h1"), (a.cpu().numpy().astype(np.float64) for a in tr.activations())))
    masks = check_masks("autograd medium 300", acts, fwd, Ef)
    assert (np.abs(lg.cpu().numpy() - fwd["logits"]) <= Ef["logits"]).all()
    ref = mg.reference_backward(w, x, c, masks=masks, fwd=fwd)
    E = mg.error_bound(w, x, c, masks=masks, fwd=fwd)
    explicit = {k: v.clone() for k, v in tr.backward(cd).items()}

    out = wh.mlp_logits(module, obs)
    assert out.shape == (rows, 9) and out.requires_grad and torch.equal(out.detach(), lg)
    (out * cd).sum().backward()
    g1 = {k: v.clone() for k, v in grads_of(module).items()}
    for k in GRADS:
        assert torch.equal(g1[k], explicit[k]), k                  # one kernel, two surfaces
        assert (np.abs(g1[k].cpu().numpy() - ref[k]) <= E[k]).all(), f"{k}: param.grad beyond the bound"
    # a second backward accumulates (the kernel overwrites its own output; autograd adds)
    (wh.mlp_logits(module, obs) * cd).sum().backward()
    for k in GRADS:
        assert torch.equal(grads_of(module)[k], g1[k] + g1[k]), k
    # torch's own autograd of the same module: each side within its bound of float64 under its own masks
    module.zero_grad(set_to_none=True)
    hooks, seen = [], {}
    for name, j in (("h0", 1), ("h1", 3)):
        hooks.append(module[j].register_forward_hook(lambda m, i, o, name=name: seen.__setitem__(name, o.detach())))
    (module(obs) * cd).sum().backward()
    for h in hooks:
        h.remove()
    tmasks = check_masks("torch medium 300", {k: v.cpu().numpy().astype(np.float64) for k, v in seen.items()}, fwd, Ef)
    tref = mg.reference_backward(w, x, c, masks=tmasks, fwd=fwd)
    tE = mg.error_bound(w, x, c, masks=tmasks, fwd=fwd)
    same = all(np.array_equal(a, b) for a, b in zip(masks, tmasks))
    print("autograd: kernel and torch masks", "agree" if same else "differ")
    for k in GRADS:
        diff = np.abs(g1[k].cpu().numpy().astype(np.float64) - grads_of(module)[k].cpu().numpy())
        allowed = E[k] + tE[k] + np.abs(ref[k] - tref[k])          # twice the bound where the masks agree
        assert (diff <= allowed).all(), f"{k}: kernel and torch autograd differ by more than both bounds"
    # an optimiser step, then the rollout network takes the new parameters through the device packer
    module.zero_grad(set_to_none=True)
    opt = torch.optim.Adam(module.parameters(), lr=1e-3)
    (wh.mlp_logits(module, obs) * cd).sum().backward()
    before = module[2].weight.detach().clone()
    opt.step()
    assert not torch.equal(before, module[2].weight.detach())
    policy = wh.policy.MLPPolicy(variant, precision="f32", device=dev)
    policy.load_weights(wh.policy.weights_of(module))
    assert policy.weights is None, "load_weights did not take the device packer"
    _, plog = policy.forward(obs, logits=True)
    new = {k: v.detach().cpu().numpy() for k, v in wh.policy.weights_of(module).items()}
    nf = mg.forward64(new, x)
    nE = mg.forward_bound(new, x, nf)["logits"]
    assert (np.abs(plog.cpu().numpy() - nf["logits"]) <= nE).all()
    assert (np.abs(wh.mlp_logits(module, obs).detach().cpu().numpy() - nf["logits"]) <= nE).all()


@pytest.mark.parametrize("variant", mx.VARIANTS)
def test_empty_batch_gives_zero_gradients(wh, variant):
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    w = mx.network(variant, mx.SEED[variant])
    module = make_module(torch, variant, w, dev)
    obs = torch.empty((0, mx.VARIANT_DIMS[variant][0]), device=dev)
    out = wh.mlp_logits(module, obs)
    assert out.shape == (0, 9)
    out.sum().backward()
    for k, g in grads_of(module).items():
        assert g is not None and g.shape == dict(wh.policy.weights_of(module))[k].shape and not g.any(), k
    tr = wh.MLPTrainer(module)
    assert tr.forward(obs).shape == (0, 9)
    mine = {k: torch.full_like(v, float("nan")) for k, v in wh.policy.weights_of(module).items()}
    got = tr.backward(torch.empty((0, 9), device=dev), out=mine)
    for k in GRADS:
        assert got[k] is mine[k] and not mine[k].any() and not torch.isnan(mine[k]).any(), k


def test_host_parameters_are_a_wrong_argument(wh):
    """Where there is a GPU, a module left on the CPU is refused as a bad argument, before any launch."""
    import torch

    module = make_module(torch, "small", mx.network("small", mx.SEED["small"]), torch.device("cpu"))
    with pytest.raises(ValueError):
        wh.mlp_logits(module, torch.zeros(4, 37))
    with pytest.raises(ValueError):
        wh.MLPTrainer(module)
