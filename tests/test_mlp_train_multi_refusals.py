"""What the multi-network training entry points refuse, with no device: wh_mlp_train_forward_multi and
wh_mlp_backward_multi are declared and exported by both libraries, wh_mlp_train_job is laid out as the
header has it, the host engine answers WH_ENOTSUP and touches no buffer, the gfx950 library checks every
rule of include/warehouse_amd.h (MLP TRAINING, the multi calls) in the header's order before it touches
the GPU -- each case here breaks two rules at once and expects the code of the earlier one -- so dummy
pointers are never dereferenced and a refused call launches nothing, and warehouse.train_forward_many /
train_backward_many / SACLearner(fused_train=...) raise ValueError for every bad argument before any
native call."""
import ctypes

import pytest

KEYS = ("w0", "b0", "w1", "b1", "w2", "b2")
DIMS = [(37, 256, 256), (82, 512, 512), (145, 1024, 256)]


@pytest.fixture(scope="module")
def nat():
    from warehouse import _native

    return _native


def job(nat, i, **kw):
    """Job i with dummy pointers of its own (one obs for all jobs, which is allowed).  Keyword fields
    replace a pointer; "w0" .. "b2" those of w, "gw0" .. "gb2" those of g."""
    b = 0x100000 * (i + 1)
    w = {k: b + 0x10 * (n + 1) for n, k in enumerate(KEYS)}
    g = {k: b + 0x5000 + 0x10 * (n + 1) for n, k in enumerate(KEYS)}
    f = dict(obs=0x1000, h0=b + 0x1000, h1=b + 0x2000, logits=b + 0x3000, dlogits=b + 0x4000, work=b + 0x6000)
    for k, v in kw.items():
        if k in w:
            w[k] = v
        elif k[0] == "g" and k[1:] in g:
            g[k[1:]] = v
        else:
            assert k in f, k
            f[k] = v
    return nat.WhMlpTrainJob(nat.WhMlpWeights(**w), f["obs"], f["h0"], f["h1"], f["logits"], f["dlogits"],
                             nat.WhMlpGrads(**g), f["work"])


def call(nat, lib, backward, desc, jobs, rows=5, nnets=None):
    """jobs: a list of WhMlpTrainJob, or None for a NULL array."""
    fn = lib.wh_mlp_backward_multi if backward else lib.wh_mlp_train_forward_multi
    arr = None if jobs is None else (nat.WhMlpTrainJob * max(1, len(jobs)))(*jobs)
    n = (0 if jobs is None else len(jobs)) if nnets is None else nnets
    return fn(ctypes.byref(desc) if desc is not None else None, n, arr, rows, None)


def test_symbols_are_declared_and_exported_by_both_libraries(nat):
    for s in ("wh_mlp_train_forward_multi", "wh_mlp_backward_multi"):
        assert s in nat.SYMBOLS
        assert hasattr(nat.lib(), s) and hasattr(nat.host_lib(), s)
    assert nat.WH_MLP_TRAIN_MAX_NETS == 4
    # wh_mlp_train_job as the header lays it out: w (six pointers), obs, h0, h1, logits, dlogits, g (six), work
    J = nat.WhMlpTrainJob
    assert ctypes.sizeof(J) == 144
    want = dict(w=0, obs=48, h0=56, h1=64, logits=72, dlogits=80, g=88, work=136)
    assert {k: getattr(J, k).offset for k in want} == want
    assert [name for name, _ in J._fields_] == list(want)


def test_header_declares_the_struct_in_the_same_order():
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "warehouse_amd.h")).read()
    assert re.search(r"#define\s+WH_MLP_TRAIN_MAX_NETS\s+4\b", text)
    body = re.search(r"typedef struct wh_mlp_train_job \{(.*?)\} wh_mlp_train_job;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"\*?\s*(\w+)\s*[,;]", body)
    assert names == ["w", "obs", "h0", "h1", "logits", "dlogits", "g", "work"]
    for s in ("wh_mlp_train_forward_multi", "wh_mlp_backward_multi"):
        assert re.search(r"int " + s + r"\(const wh_mlp_desc\* d, int32_t nnets, const wh_mlp_train_job\* jobs,\s*"
                         r"int64_t rows, void\* stream\);", text), s


def test_host_engine_answers_enotsup_and_touches_nothing(nat):
    import torch

    lib = nat.host_lib()
    desc = nat.WhMlpDesc(37, 256, 256, 9, nat.WH_MLP_F32)
    bufs = [torch.full((4096,), 0xA5, dtype=torch.uint8) for _ in range(36)]
    jobs = []
    for i in range(2):
        p = [b.data_ptr() for b in bufs[18 * i:18 * (i + 1)]]
        jobs.append(nat.WhMlpTrainJob(nat.WhMlpWeights(*p[0:6]), p[6], p[7], p[8], p[9], p[10], nat.WhMlpGrads(*p[11:17]),
                                      p[17]))
    for backward in (False, True):
        for rows in (1, 0):
            assert call(nat, lib, backward, desc, jobs, rows=rows) == nat.WH_ENOTSUP
        assert call(nat, lib, backward, desc, [], rows=1) == nat.WH_ENOTSUP
    assert all(bool((b == 0xA5).all()) for b in bufs)


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("dims", DIMS)
def test_refusals_of_the_device_library_need_no_device(nat, dims, backward):
    lib = nat.lib()
    E, N, OK = nat.WH_EINVAL, nat.WH_ENOTSUP, nat.WH_OK
    OVER = (1 << 24) + 1
    desc = nat.WhMlpDesc(*dims, 9, nat.WH_MLP_F32)
    bad_descs = (nat.WhMlpDesc(dims[0] + 1, dims[1], dims[2], 9, 1), nat.WhMlpDesc(dims[0], dims[2] * 2, dims[1], 9, 1),
                 nat.WhMlpDesc(*dims, 8, 1), nat.WhMlpDesc(*dims, 9, nat.WH_MLP_BF16), nat.WhMlpDesc(*dims, 9, 7))
    own = "dlogits" if backward else "logits"          # the direction's own required pointer
    dup = dict(work=0x100000 + 0x6000) if backward else dict(h0=0x100000 + 0x1000)   # job 1 given job 0's buffer

    def run(d, jobs, **kw):
        return call(nat, lib, backward, d, jobs, **kw)

    two = [job(nat, 0), job(nat, 1)]
    # what is accepted without a launch: no jobs; (forward) the empty batch
    assert run(desc, []) == OK and run(desc, None) == OK
    if not backward:
        assert run(desc, two, rows=0) == OK
        assert run(desc, [job(nat, i) for i in range(4)], rows=0) == OK

    # 1. d == NULL, with: a bad row count, a bad count of jobs, a NULL array, a job's NULL pointer
    assert run(None, two) == E
    assert run(None, two, rows=-1) == E
    assert run(None, None, nnets=9) == E
    assert run(None, [job(nat, 0, obs=None)]) == E
    # 2. the shape / out_dim / precision (WH_ENOTSUP), with each later rule (all WH_EINVAL) broken too
    for bad in bad_descs:
        assert run(bad, two) == N
        assert run(bad, two, rows=-1) == N
        assert run(bad, two, rows=OVER) == N
        assert run(bad, None, nnets=5) == N
        assert run(bad, None, nnets=-1) == N
        assert run(bad, None, nnets=2) == N
        assert run(bad, [job(nat, 0, w0=None)]) == N
        assert run(bad, [job(nat, 0, **{own: None})]) == N
        assert run(bad, [job(nat, 0), job(nat, 1, **dup)]) == N
        if backward:
            assert run(bad, [job(nat, 0, work=0x60001)]) == N
    # 3. rows, with a count of jobs whose NULL array would be read, and with jobs that hold NULL pointers:
    #    the code is WH_EINVAL either way, and nothing of the array is read (ASan holds that)
    for rows in (-1, OVER):
        assert run(desc, two, rows=rows) == E
        assert run(desc, None, nnets=5, rows=rows) == E
        assert run(desc, [], rows=rows) == E
        assert run(desc, [job(nat, 0, obs=None)], rows=rows) == E
    # 4. the count of jobs, with jobs that break a later rule
    assert run(desc, two, nnets=-1) == E
    assert run(desc, [job(nat, i) for i in range(5)]) == E
    assert run(desc, [job(nat, i, obs=None) for i in range(5)]) == E
    assert run(desc, None, nnets=1) == E
    assert run(desc, None, nnets=4, rows=0) == E
    # 5. every job's own pointers, in every position, also for the empty batch, also beside a shared buffer
    for rows in (5, 0):
        for at in range(4):
            def jobs_with(**kw):
                return [job(nat, i, **(kw if i == at else {})) for i in range(4)]
            for k in KEYS:
                assert run(desc, jobs_with(**{k: None}), rows=rows) == E
                if backward:
                    assert run(desc, jobs_with(**{"g" + k: None}), rows=rows) == E
            for k in ("obs", "h0", "h1", own):
                assert run(desc, jobs_with(**{k: None}), rows=rows) == E
            if backward:
                assert run(desc, jobs_with(work=None), rows=rows) == E
                for off in (1, 4, 8):
                    assert run(desc, jobs_with(work=0x100000 * (at + 1) + 0x6000 + off), rows=rows) == E
        assert run(desc, [job(nat, 0), job(nat, 1, w2=None, **dup)], rows=rows) == E
    # 6. two jobs with one output buffer: every pair, every field
    fields = ["work"] + ["g" + k for k in KEYS] if backward else ["h0", "h1", "logits"]
    for hi in range(1, 4):
        for lo in range(hi):
            for f in fields:
                src = job(nat, lo)
                value = getattr(src.g, f[1:]) if f[0] == "g" else getattr(src, f)
                jobs = [job(nat, i, **({f: value} if i == hi else {})) for i in range(4)]
                assert run(desc, jobs) == E, (hi, lo, f)
                if not backward:
                    assert run(desc, jobs, rows=0) == E, (hi, lo, f)
    # the fields of the other direction are not looked at, and shared inputs are no defect
    if backward:
        assert run(desc, None, nnets=0) == OK
    else:
        other = dict(dlogits=None, work=3, **{"g" + k: None for k in KEYS})
        assert run(desc, [job(nat, 0, **other), job(nat, 1, **other)], rows=0) == OK
        shared = {k: 0x100000 + 0x10 * (n + 1) for n, k in enumerate(KEYS)}
        assert run(desc, [job(nat, 0), job(nat, 1, **shared)], rows=0) == OK


def modules(torch):
    def seq(i, a, b):
        L = torch.nn.Linear
        return torch.nn.Sequential(L(i, a), torch.nn.ReLU(), L(a, b), torch.nn.ReLU(), L(b, 9))
    return seq


def bare_trainer(train, torch, module, dims=(37, 256, 256), device="cpu"):
    """An MLPTrainer put together without its constructor's device check (there is no device here)."""
    t = train.MLPTrainer.__new__(train.MLPTrainer)
    t.module, t.dims, t.device, t._buf, t._obs = module, dims, torch.device(device), {}, None
    return t


def test_python_surface_refuses_before_any_native_call(nat, monkeypatch):
    import torch
    import warehouse
    from warehouse import train

    def no_native(*a, **k):
        raise AssertionError("a refused call reached the native library")
    monkeypatch.setattr(train.nat, "lib", no_native)
    seq = modules(torch)
    small = [bare_trainer(train, torch, seq(37, 256, 256)) for _ in range(5)]
    medium = bare_trainer(train, torch, seq(82, 512, 512), dims=(82, 512, 512))
    elsewhere = bare_trainer(train, torch, seq(37, 256, 256).to("meta"), device="meta")
    x = torch.zeros(4, 37)
    fwd, bwd = warehouse.train_forward_many, warehouse.train_backward_many
    assert fwd([], x) == [] and fwd([], []) == [] and bwd([], []) == []
    bad_forward = [
        (small, x),                                       # more than four trainers
        ([small[0], medium], x),                          # mixed shapes
        ([small[0], elsewhere], x),                       # mixed devices
        ([small[0], small[1]], [x, torch.zeros(5, 37)]),  # differing row counts
        ([small[0], small[1], small[0]], x),              # one trainer listed twice
        ([small[0], small[1]], [x]),                      # obs: one tensor, or one per trainer
        ([small[0], object()], x),
        ([small[0]], torch.zeros(4, 36)),
        ([small[0]], torch.zeros(4, 37, dtype=torch.float64)),
        ([small[0]], torch.zeros(4, 37, requires_grad=True)),
        ([small[0], small[1]], [x, torch.zeros(4, 74)[:, ::2]]),
    ]
    for trainers, obs in bad_forward:
        with pytest.raises(ValueError):
            fwd(trainers, obs)
    assert all(t._obs is None for t in small), "a refused forward left no obs behind"
    dz = torch.zeros(4, 9)
    with pytest.raises(ValueError):
        bwd([small[0]], [dz])                             # no forward yet
    for t in small:
        t._obs = x
    medium._obs, elsewhere._obs = torch.zeros(4, 82), torch.zeros(4, 37, device="meta")
    small[4]._obs = torch.zeros(5, 37)
    ok = {k: torch.zeros_like(v) for k, v in train.weights_of(small[0].module).items()}
    bad_backward = [
        (small, [dz] * 5, None),
        ([small[0], medium], [dz, dz], None),
        ([small[0], elsewhere], [dz, dz], None),
        ([small[0], small[4]], [dz, torch.zeros(5, 9)], None),   # the forwards had differing row counts
        ([small[0], small[0]], [dz, dz], None),
        ([small[0], small[1]], [dz], None),
        ([small[0], small[1]], dz, None),                        # dlogits is a list
        ([small[0], small[1]], [dz, torch.zeros(5, 9)], None),
        ([small[0], small[1]], [dz, torch.zeros(4, 8)], None),
        ([small[0], small[1]], [dz, torch.zeros(4, 9, dtype=torch.float64)], None),
        ([small[0], small[1]], [dz, dz], [ok]),
        ([small[0], small[1]], [dz, dz], [ok, dict(ok, w1=torch.zeros(256, 255))]),
        ([small[0], small[1]], [dz, dz], [ok, {k: v for k, v in ok.items() if k != "b0"}]),
        ([small[0], small[1]], [dz, dz], [ok, ok]),              # two trainers' gradients in one tensor
    ]
    for trainers, dzs, out in bad_backward:
        with pytest.raises(ValueError):
            bwd(trainers, dzs, out)


def test_learner_refuses_a_bad_fused_train(nat, monkeypatch):
    import torch
    import warehouse
    from warehouse import learner, sac, train

    def no_native(*a, **k):
        raise AssertionError("a refused call reached the native library")
    monkeypatch.setattr(train.nat, "lib", no_native)
    seq = modules(torch)
    mods = [seq(37, 256, 256) for _ in range(3)]
    for bad in ("yes", 1, 0, 2.0, [True]):
        with pytest.raises(ValueError, match="fused_train"):
            warehouse.SACLearner(*mods, rollout_policy=None, critic=None, log_alpha=torch.zeros(1), fused_train=bad)
    # modules of two shapes cannot share a launch: fused_train=True says so (the trainers built without a device)
    monkeypatch.setattr(learner, "MLPTrainer",
                        lambda m: bare_trainer(train, torch, m, dims=train._network(m)[1]))
    critic = sac.SACCritic.__new__(sac.SACCritic)
    critic.q2 = object()
    with pytest.raises(ValueError, match="one shape"):
        warehouse.SACLearner(mods[0], mods[1], seq(82, 512, 512), rollout_policy=None, critic=critic,
                             log_alpha=torch.zeros(1), fused_train=True)
