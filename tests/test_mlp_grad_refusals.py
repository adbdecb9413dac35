"""What the MLP training entry points refuse, with no device: wh_mlp_train_query, wh_mlp_train_forward and
wh_mlp_backward are declared and exported by both libraries, the host engine answers WH_ENOTSUP like its
other wh_mlp_* entry points, the gfx950 library checks every rule of include/warehouse_amd.h (MLP
TRAINING) -- in the header's order -- before it touches the GPU, so dummy pointers are never dereferenced
and a refused call launches nothing, and warehouse.mlp_logits / MLPTrainer raise ValueError for every bad
argument before any native call."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def nat():
    from warehouse import _native

    return _native


def six(nat, base, **kw):
    f = {k: base + 0x1000 * i for i, k in enumerate(("w0", "b0", "w1", "b1", "w2", "b2"))}
    f.update(kw)
    return nat.WhMlpWeights(**f)


def ref(s):
    return ctypes.byref(s) if s is not None else None


def fwd(nat, lib, desc, w="ok", rows=5, obs=0x20000, h0=0x30000, h1=0x40000, logits=0x50000):
    w = six(nat, 0x100000) if isinstance(w, str) else w
    return lib.wh_mlp_train_forward(ref(desc), ref(w), rows, obs, h0, h1, logits, None)


def bwd(nat, lib, desc, w="ok", rows=5, obs=0x20000, h0=0x30000, h1=0x40000, dz=0x50000, g="ok", work=0x60000):
    w = six(nat, 0x100000) if isinstance(w, str) else w
    g = six(nat, 0x200000) if isinstance(g, str) else g
    return lib.wh_mlp_backward(ref(desc), ref(w), rows, obs, h0, h1, dz, ref(g), work, None)


def test_symbols_are_declared_and_exported_by_both_libraries(nat):
    for s in ("wh_mlp_train_query", "wh_mlp_train_forward", "wh_mlp_backward"):
        assert s in nat.SYMBOLS
        assert hasattr(nat.lib(), s) and hasattr(nat.host_lib(), s)
    # wh_mlp_weights / wh_mlp_grads as the header lays them out: six pointers, w0 b0 w1 b1 w2 b2
    for S in (nat.WhMlpWeights, nat.WhMlpGrads):
        assert ctypes.sizeof(S) == 48
        assert [getattr(S, k).offset for k in ("w0", "b0", "w1", "b1", "w2", "b2")] == [0, 8, 16, 24, 32, 40]
    assert nat.WH_MLP_TRAIN_MAX_ROWS == 1 << 24


def test_host_engine_answers_enotsup_and_touches_nothing(nat):
    import torch

    lib = nat.host_lib()
    desc = nat.WhMlpDesc(37, 256, 256, 9, nat.WH_MLP_F32)
    bufs = [torch.full((4096,), 0xA5, dtype=torch.uint8) for _ in range(18)]
    p = [b.data_ptr() for b in bufs]
    w = nat.WhMlpWeights(*p[0:6])
    g = nat.WhMlpWeights(*p[6:12])
    n = ctypes.c_int64(-7)
    assert lib.wh_mlp_train_query(ctypes.byref(desc), 1, ctypes.byref(n)) == nat.WH_ENOTSUP and n.value == -7
    assert lib.wh_mlp_train_forward(ctypes.byref(desc), ctypes.byref(w), 1, p[12], p[13], p[14], p[15], None) == nat.WH_ENOTSUP
    assert lib.wh_mlp_backward(ctypes.byref(desc), ctypes.byref(w), 1, p[12], p[13], p[14], p[15], ctypes.byref(g), p[16],
                               None) == nat.WH_ENOTSUP
    assert lib.wh_mlp_backward(ctypes.byref(desc), ctypes.byref(w), 0, p[12], p[13], p[14], p[15], ctypes.byref(g), p[16],
                               None) == nat.WH_ENOTSUP
    assert all(bool((b == 0xA5).all()) for b in bufs)


def test_query_sizes_and_refusals(nat):
    lib = nat.lib()
    E, N, OK = nat.WH_EINVAL, nat.WH_ENOTSUP, nat.WH_OK
    n = ctypes.c_int64()
    for dims in ((37, 256, 256), (82, 512, 512), (145, 1024, 256)):
        desc = nat.WhMlpDesc(*dims, 9, nat.WH_MLP_F32)
        last = 0
        for rows in (0, 1, 33, 512, 513, 4096, 1 << 24):
            assert lib.wh_mlp_train_query(ctypes.byref(desc), rows, ctypes.byref(n)) == OK
            # room for dH1 and dH0 at least, a multiple of 16, never 0, growing with rows
            assert n.value >= max(16, 4 * rows * (dims[1] + dims[2])) and n.value % 16 == 0 and n.value >= last
            last = n.value
        assert lib.wh_mlp_train_query(ctypes.byref(desc), 5, None) == OK
        assert lib.wh_mlp_train_query(ctypes.byref(desc), -1, ctypes.byref(n)) == E
        assert lib.wh_mlp_train_query(ctypes.byref(desc), (1 << 24) + 1, ctypes.byref(n)) == E
    assert lib.wh_mlp_train_query(None, 5, ctypes.byref(n)) == E
    for bad in (nat.WhMlpDesc(83, 512, 512, 9, 1), nat.WhMlpDesc(82, 512, 256, 9, 1), nat.WhMlpDesc(82, 512, 512, 8, 1),
                nat.WhMlpDesc(82, 512, 512, 9, nat.WH_MLP_BF16), nat.WhMlpDesc(82, 512, 512, 9, 7)):
        assert lib.wh_mlp_train_query(ctypes.byref(bad), 5, ctypes.byref(n)) == N
        assert lib.wh_mlp_train_query(ctypes.byref(bad), -1, ctypes.byref(n)) == N     # the desc comes before rows


@pytest.mark.parametrize("dims", [(37, 256, 256), (82, 512, 512), (145, 1024, 256)])
def test_refusals_of_the_device_library_need_no_device(nat, dims):
    lib = nat.lib()
    E, N, OK = nat.WH_EINVAL, nat.WH_ENOTSUP, nat.WH_OK
    desc = nat.WhMlpDesc(*dims, 9, nat.WH_MLP_F32)
    calls = (lambda d, **kw: fwd(nat, lib, d, **kw), lambda d, **kw: bwd(nat, lib, d, **kw))
    for call in calls:
        # d, then the shape and out_dim, then the precision: each before rows and every pointer
        assert call(None) == E
        assert call(None, rows=-1, w=None) == E
        for bad in (nat.WhMlpDesc(dims[0] + 1, dims[1], dims[2], 9, 1), nat.WhMlpDesc(dims[0], dims[2] * 2, dims[1], 9, 1),
                    nat.WhMlpDesc(*dims, 8, 1), nat.WhMlpDesc(*dims, 9, nat.WH_MLP_BF16), nat.WhMlpDesc(*dims, 9, 7)):
            assert call(bad) == N
            assert call(bad, rows=-1) == N
            assert call(bad, w=None, obs=None) == N
        # rows < 0 before the pointers
        assert call(desc, rows=-1) == E
        assert call(desc, rows=-1, w=None, obs=None) == E
        # the pointers: also refused for the empty batch
        for rows in (5, 0):
            assert call(desc, rows=rows, w=None) == E
            for k in ("w0", "b0", "w1", "b1", "w2", "b2"):
                assert call(desc, rows=rows, w=six(nat, 0x100000, **{k: None})) == E
            for k in ("obs", "h0", "h1"):
                assert call(desc, rows=rows, **{k: None}) == E
        # the row limit comes last
        assert call(desc, rows=(1 << 24) + 1) == E
        assert call(desc, rows=(1 << 24) + 1, obs=None) == E
    f, b = calls
    for rows in (5, 0):
        assert f(desc, rows=rows, logits=None) == E
        assert b(desc, rows=rows, dz=None) == E
        assert b(desc, rows=rows, g=None) == E
        for k in ("w0", "b0", "w1", "b1", "w2", "b2"):
            assert b(desc, rows=rows, g=six(nat, 0x200000, **{k: None})) == E
        assert b(desc, rows=rows, work=None) == E
        for off in (1, 4, 8):
            assert b(desc, rows=rows, work=0x60000 + off) == E
    assert b(desc, rows=-1, work=0x60001) == E
    assert b(nat.WhMlpDesc(*dims, 9, nat.WH_MLP_BF16), work=0x60001) == N      # the precision before the alignment
    # the empty forward launches nothing and needs no device
    assert f(desc, rows=0) == OK


def modules(torch):
    def seq(i, a, b, o=9, bias=True):
        L = torch.nn.Linear
        return torch.nn.Sequential(L(i, a), torch.nn.ReLU(), L(a, b), torch.nn.ReLU(), L(b, o, bias=bias))
    return seq


def bare_trainer(train, torch, module):
    """An MLPTrainer put together without its constructor's device check (there is no device here)."""
    t = train.MLPTrainer.__new__(train.MLPTrainer)
    t.module, t.dims, t.device, t._buf, t._obs = module, (37, 256, 256), torch.device("cpu"), {}, None
    return t


@pytest.mark.parametrize("surface", ["mlp_logits", "MLPTrainer"])
def test_python_surface_refuses_before_any_native_call(nat, surface, monkeypatch):
    import torch
    import warehouse
    from warehouse import train

    def no_native(*a, **k):
        raise AssertionError("a refused call reached the native library")
    monkeypatch.setattr(train.nat, "lib", no_native)
    seq = modules(torch)

    def run(module, obs, bare=False):
        if surface == "mlp_logits":
            return warehouse.mlp_logits(module, obs)
        if bare:        # (the constructor asks for the device; forward's own checks on a trainer without one)
            return bare_trainer(train, torch, module).forward(obs)
        return warehouse.MLPTrainer(module).forward(obs)

    good = seq(37, 256, 256)
    x = torch.zeros(4, 37)
    bad_modules = [seq(36, 256, 256), seq(37, 256, 128), seq(82, 512, 256), seq(37, 256, 256, o=8),
                   seq(37, 256, 256, bias=False), seq(37, 256, 256).double(), seq(37, 256, 256).half(),
                   torch.nn.Sequential(torch.nn.Linear(37, 256), torch.nn.Tanh(), torch.nn.Linear(256, 256),
                                       torch.nn.ReLU(), torch.nn.Linear(256, 9)),
                   torch.nn.Sequential(torch.nn.Linear(37, 256), torch.nn.ReLU(), torch.nn.Linear(256, 9))]
    strided = seq(37, 256, 256)
    strided[2].weight = torch.nn.Parameter(torch.zeros(256, 512)[:, ::2])       # not contiguous
    bad_modules.append(strided)
    meta = seq(37, 256, 256)
    meta[4] = torch.nn.Linear(256, 9, device="meta")                             # parameters on two devices
    bad_modules.append(meta)
    for m in bad_modules:
        with pytest.raises(ValueError):
            run(m, x)
    bad_obs = [torch.zeros(4, 36), torch.zeros(4, 37, dtype=torch.float64), torch.zeros(4, 74)[:, ::2], torch.zeros(37),
               torch.zeros(2, 2, 37), torch.zeros(4, 37, requires_grad=True), torch.zeros(4, 37, device="meta"),
               [[0.0] * 37]]
    for o in bad_obs:
        with pytest.raises(ValueError):
            run(good, o, bare=True)
    if not torch.cuda.is_available():
        # every argument is fine: the package's usual error for a missing device (no CPU fallback)
        with pytest.raises(RuntimeError, match="no HIP device"):
            run(good, x)


def test_trainer_backward_refuses_bad_gradients_without_a_device(nat, monkeypatch):
    """MLPTrainer.backward's own checks."""
    import torch
    from warehouse import train

    def no_native(*a, **k):
        raise AssertionError("a refused call reached the native library")
    monkeypatch.setattr(train.nat, "lib", no_native)
    t = bare_trainer(train, torch, modules(torch)(37, 256, 256))
    with pytest.raises(ValueError):
        t.backward(torch.zeros(4, 9))                       # no forward yet
    t._obs = torch.zeros(4, 37)
    for dz in (torch.zeros(4, 8), torch.zeros(5, 9), torch.zeros(4, 9, dtype=torch.float64), torch.zeros(4, 18)[:, ::2],
               torch.zeros(4, 9, device="meta")):
        with pytest.raises(ValueError):
            t.backward(dz)
    ok = {k: torch.zeros_like(v) for k, v in train.weights_of(t.module).items()}
    for bad in (dict(ok, w1=torch.zeros(256, 255)), dict(ok, b2=torch.zeros(9, dtype=torch.float64)),
                {k: v for k, v in ok.items() if k != "b0"}, dict(ok, extra=torch.zeros(1))):
        with pytest.raises(ValueError):
            t.backward(torch.zeros(4, 9), out=bad)
