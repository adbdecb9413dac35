"""The SAC forward half on the GPU: wh_mlp_pack_device (k_mlp_pack, csrc/mlp_pack.h) byte for byte
against wh_mlp_pack, wh_sac_td (k_sac_td, csrc/sac.h) against the float64 model of tests/sac_cases.py
within the bounds stated there, and warehouse.SACCritic end to end on a wrapped prioritized ring.
tests/test_sac_cpu.py runs the wh_sac_td bodies on the host engine.

Largest wh_sac_td errors seen on the device, as fractions of the bounds (y, td_rows, td):
0.046, 0.051, 0.0107; on the peaked-policy case 0.031, 0.025, 0.0053."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import sac_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("w0", "b0", "w1", "b1", "w2", "b2")


@pytest.fixture(scope="module")
def nat():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from warehouse import _native

    return _native


@pytest.fixture(scope="module")
def wh():
    import warehouse
    import warehouse.policy  # noqa: F401
    import warehouse.sac  # noqa: F401

    return warehouse


def device_weights(w):
    import torch

    return {k: torch.as_tensor(w[k]).to("cuda:0").contiguous() for k in KEYS}


# ----------------------------------------------------------------------------- pack
@pytest.mark.parametrize("precision", ["bf16", "f32"])
@pytest.mark.parametrize("variant", ["small", "medium", "large"])
def test_device_blob_equals_host_blob(nat, variant, precision):
    sc.case_pack_equal(nat, variant, precision, seed=3)


def test_device_blob_equals_host_blob_on_the_legacy_route():
    """bf16 Medium with WH_MLP_LEGACY=1 (the 32x32x16 blob): the choice is a process-wide static,
    so a fresh child process."""
    env = dict(os.environ, WH_MLP_LEGACY="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sac_cases.py")], capture_output=True, text=True,
                       env=env, timeout=120)
    assert r.returncode == 0 and "LEGACY PACK OK" in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_pack_device_refusals_on_the_device(nat):
    import torch

    lib = nat.lib()
    desc = nat.WhMlpDesc(37, 256, 256, 9, nat.WH_MLP_BF16)
    w = device_weights(sc.pack_weights(37, 256, 256, 1))
    nbytes = ctypes.c_int64()
    assert lib.wh_mlp_query(ctypes.byref(desc), ctypes.byref(nbytes)) == nat.WH_OK
    blob = torch.full((nbytes.value + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
    ptrs = [w[k].data_ptr() for k in KEYS] + [blob.data_ptr()]
    stream = nat.stream_of(torch.device("cuda:0"))
    assert lib.wh_mlp_pack_device(None, *ptrs, stream) == nat.WH_EINVAL
    for i in range(7):
        p = list(ptrs)
        p[i] = None
        assert lib.wh_mlp_pack_device(ctypes.byref(desc), *p, stream) == nat.WH_EINVAL, i
    assert lib.wh_mlp_pack_device(ctypes.byref(desc), *ptrs[:6], blob.data_ptr() + 4, stream) == nat.WH_EINVAL
    bad = nat.WhMlpDesc(38, 256, 256, 9, nat.WH_MLP_BF16)
    assert lib.wh_mlp_pack_device(ctypes.byref(bad), *ptrs, stream) == nat.WH_ENOTSUP
    host = [torch.zeros(64) for _ in range(7)]
    assert nat.host_lib().wh_mlp_pack_device(ctypes.byref(desc), *[t.data_ptr() for t in host], None) == nat.WH_ENOTSUP
    torch.cuda.synchronize()
    assert bool((blob == 0xA5).all()), "a refused call wrote to the blob"


def test_load_weights_on_a_side_stream_gives_the_host_paths_logits(wh):
    """load_weights from device tensors on a non-default stream, then forward_x there: the logits
    equal, at tolerance 0, those of a network constructed from the same values through the host path."""
    import torch

    w = wh.policy.init_weights(37, 256, 256, seed=21)
    ref = wh.policy.MLPPolicy("small", weights=w)
    net = wh.policy.MLPPolicy("small", seed=99)
    env = wh.BatchedWarehouse("small", 40, 4, seed=2, device="cuda:0")
    env.reset()
    x = env.observe_x().clone()
    rows = 40 * 4
    _, want = ref.forward_x(x, rows, logits=True)
    _, before = net.forward_x(x, rows, logits=True)
    assert not torch.equal(before, want)
    wd = device_weights(w)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        net.load_weights(wd)
        _, got = net.forward_x(x, rows, logits=True)
    side.synchronize()
    assert net.weights is None
    assert torch.equal(got, want)
    assert torch.equal(net.packed, ref.packed)


def test_load_weights_twice_the_second_set_wins_and_the_host_path_refreshes_weights(wh):
    import torch

    a = wh.policy.init_weights(82, 512, 512, seed=1)
    b = wh.policy.init_weights(82, 512, 512, seed=2)
    net = wh.policy.MLPPolicy("medium", seed=7)
    net.load_weights(device_weights(a))
    net.load_weights(device_weights(b))
    assert torch.equal(net.packed, wh.policy.MLPPolicy("medium", weights=b).packed) and net.weights is None
    net.load_weights(a)                                       # numpy: the host path
    assert torch.equal(net.packed, wh.policy.MLPPolicy("medium", weights=a).packed)
    assert net.weights is not None and np.array_equal(net.weights["w1"], a["w1"])
    bad = dict(device_weights(a), w1=torch.zeros((512, 511), device="cuda:0"))
    with pytest.raises(ValueError, match="w1"):
        net.load_weights(bad)
    with pytest.raises(ValueError, match="b2"):
        net.load_weights(dict(a, b2=np.zeros(8, np.float32)))
    f32 = wh.policy.MLPPolicy("medium", seed=7, precision="f32")
    f32.load_weights(device_weights(b))
    assert torch.equal(f32.packed, wh.policy.MLPPolicy("medium", weights=b, precision="f32").packed)


def test_copy_from_and_weights_of(wh):
    import torch

    src = wh.policy.MLPPolicy("small", seed=4)
    dst = wh.policy.MLPPolicy("small", seed=5)
    assert not torch.equal(dst.packed, src.packed)
    dst.copy_from(src)
    assert torch.equal(dst.packed, src.packed) and dst.packed.data_ptr() != src.packed.data_ptr()
    with pytest.raises(ValueError):
        dst.copy_from(wh.policy.MLPPolicy("medium", seed=4))
    with pytest.raises(ValueError):
        dst.copy_from(wh.policy.MLPPolicy("small", seed=4, precision="f32"))
    mod = torch.nn.Sequential(torch.nn.Linear(37, 256), torch.nn.ReLU(), torch.nn.Linear(256, 256), torch.nn.ReLU(),
                              torch.nn.Linear(256, 9)).to("cuda:0")
    w = wh.policy.weights_of(mod)
    for i, m in enumerate((mod[0], mod[2], mod[4])):
        assert w[f"w{i}"].data_ptr() == m.weight.data_ptr() and w[f"b{i}"].data_ptr() == m.bias.data_ptr()
    dst.load_weights(w)
    assert dst.weights is None
    want = wh.policy.MLPPolicy("small", weights={k: v.cpu().numpy() for k, v in w.items()})
    assert torch.equal(dst.packed, want.packed)


# ----------------------------------------------------------------------------- wh_sac_td
@pytest.mark.parametrize("M", sc.MS)
@pytest.mark.parametrize("NA", sc.NAS)
def test_td_against_the_float64_model(nat, NA, M):
    worst = sc.case_td(nat, nat.lib(), "cuda:0", NA, M)
    print("device NA", NA, "M", M, "errors / bounds", worst)


def test_refusals_on_the_device(nat):
    assert sc.case_refusals(nat, nat.lib(), host=False) == sc.case_refusals(nat, nat.host_lib(), host=True)


# ----------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def e2e(wh):
    """Small-4, B = 8, a prioritized ring of 4 slots wrapped by six recorded steps, 16 samples with
    duplicates and one planted out-of-ring index, five bf16 networks."""
    import torch
    from replay_cases import place_near_end

    env = wh.BatchedWarehouse("small", 8, 4, seed=11, device="cuda:0")
    place_near_end(env)
    buf = wh.ReplayBuffer(env, capacity=4, prioritized=True)
    for _ in range(6):
        buf.step(env.policy("greedy", 0.3))
    assert buf.filled == 4 and buf.cursor == 2
    rng = np.random.default_rng(5)
    idx = rng.integers(0, len(buf), 16)
    done = np.flatnonzero(buf.dones.cpu().numpy().reshape(-1))
    assert len(done), "no recorded episode end in the ring"
    idx[0], idx[1] = done[0], done[-1]                        # finished episodes (mask_dones)
    idx[3] = idx[9]
    idx[6] = len(buf) + 7                                     # outside the ring: n = -1
    batch = {k: v.clone() for k, v in buf.sample(16, idx=idx, rows=False, fragments=True).items()}
    nets = [wh.policy.MLPPolicy("small", seed=30 + i) for i in range(5)]
    torch.cuda.synchronize()
    return env, buf, batch, nets, idx


def logits_of(net, frag, rows):
    return net.forward_x(frag, rows, logits=True)[1].cpu().numpy()


@pytest.mark.parametrize("mask_dones", [False, True])
def test_critic_td_against_the_model_on_the_networks_own_logits(wh, e2e, mask_dones):
    env, buf, batch, nets, idx = e2e
    policy, q1, q2, q1t, q2t = nets
    critic = wh.SACCritic(policy, q1, q2, q1t, q2t, alpha=0.2, gamma=0.9, n_step=3, mask_dones=mask_dones)
    out = {k: v.cpu().numpy() for k, v in critic.td(batch).items()}
    M, NA = 16, 4
    rows = M * NA
    inp = dict(pi_next=logits_of(policy, batch["next_xfrag"], rows), q1t_next=logits_of(q1t, batch["next_xfrag"], rows),
               q2t_next=logits_of(q2t, batch["next_xfrag"], rows), q1=logits_of(q1, batch["xfrag"], rows),
               q2=logits_of(q2, batch["xfrag"], rows), actions=batch["actions"].cpu().numpy(),
               rewards=batch["rewards"].cpu().numpy(), dones=batch["dones"].cpu().numpy(), n=batch["n"].cpu().numpy())
    assert inp["n"][6] == -1 and (inp["n"][np.arange(M) != 6] == 4).all()
    assert mask_dones is False or inp["dones"].any(), "the batch holds no finished episode"
    discount = 0.9 ** 3
    y, td_rows, td = sc.model(inp, NA, alpha=0.2, discount=discount, mask_dones=int(mask_dones))
    L = float(np.abs(inp["pi_next"]).max())
    Qm = float(max(np.abs(inp[k]).max() for k in ("q1t_next", "q2t_next", "q1", "q2")))
    by, btd = sc.bounds(NA, 0.2, discount, rmax=float(np.abs(inp["rewards"]).max()), L=L, Qm=Qm)
    assert np.abs(out["y"] - y).max() <= by and np.abs(out["td_rows"] - td_rows).max() <= by
    assert np.abs(out["td"] - td).max() <= btd
    assert out["td"][6] == 0 and not out["y"][6].any() and not out["td_rows"][6].any()
    assert (out["td"][np.arange(M) != 6] > 0).all()
    # single Q through the class: q2 = q2_target = None
    single = wh.SACCritic(policy, q1, None, q1t, None, alpha=0.0, gamma=0.9, mask_dones=mask_dones)
    got = {k: v.cpu().numpy() for k, v in single.td(batch).items()}
    y1, tr1, td1 = sc.model(dict(inp, q2=None, q2t_next=None), NA, alpha=0.0, discount=0.9, mask_dones=int(mask_dones))
    by1, btd1 = sc.bounds(NA, 0.0, 0.9, rmax=float(np.abs(inp["rewards"]).max()), L=L, Qm=Qm)
    assert np.abs(got["y"] - y1).max() <= by1 and np.abs(got["td_rows"] - tr1).max() <= by1
    assert np.abs(got["td"] - td1).max() <= btd1


def test_targets_equal_td_bit_for_bit_and_out_is_the_callers(wh, e2e):
    import torch

    env, buf, batch, nets, idx = e2e
    critic = wh.SACCritic(*nets, alpha=0.2, gamma=0.99)
    y = critic.td(batch)["y"].clone()
    t = critic.targets(batch)
    assert set(t) == {"y"} and torch.equal(t["y"], y)
    mine = dict(td=torch.full((16,), -1.0, device="cuda:0"))
    got = critic.td(batch, out=mine)
    assert got["td"].data_ptr() == mine["td"].data_ptr() and torch.equal(mine["td"], critic.td(batch)["td"])
    with pytest.raises(ValueError):
        critic.targets(batch, out=mine)
    critic.alpha = 0.0                                        # a plain attribute
    assert not torch.equal(critic.targets(batch)["y"], y)
    with pytest.raises(ValueError):
        wh.SACCritic(nets[0], nets[1], nets[2], nets[3], None, alpha=0.2)
    # f32 networks read the rows
    rows_batch = buf.sample(16, idx=idx, rows=True)
    f32 = [wh.policy.MLPPolicy("small", seed=30 + i, precision="f32") for i in range(5)]
    c32 = wh.SACCritic(*f32, alpha=0.2, gamma=0.99)
    out = c32.td(rows_batch)
    assert tuple(out["y"].shape) == (16, 4) and float(out["td"][6]) == 0.0
    with pytest.raises(ValueError, match="rows"):
        c32.td(batch)


def test_sync_targets_copies_both_blobs(wh):
    import torch

    nets = [wh.policy.MLPPolicy("small", seed=40 + i) for i in range(5)]
    critic = wh.SACCritic(*nets, alpha=0.2)
    assert not torch.equal(nets[3].packed, nets[1].packed)
    critic.sync_targets()
    assert torch.equal(nets[3].packed, nets[1].packed) and torch.equal(nets[4].packed, nets[2].packed)


def test_td_errors_become_the_rings_priorities(wh, e2e):
    """update_priorities(idx_out, td), then the same entries read back: their leaves equal
    quantise((|td| + eps) ** alpha), the largest duplicate winning; the invalid sample leaves the
    tree alone."""
    import torch
    from prio_cases import quantise

    env, buf, batch, nets, idx = e2e
    critic = wh.SACCritic(*nets, alpha=0.2, gamma=0.99)
    out = critic.td(batch)
    valid = (idx >= 0) & (idx < len(buf))
    np.testing.assert_array_equal(batch["idx_out"].cpu().numpy()[valid], idx[valid])
    before = buf.prio_leaf.cpu().numpy().view(np.uint32).copy()
    buf.update_priorities(batch["idx_out"], out["td"])
    again = buf.sample(16, idx=batch["idx_out"], fragments=True)
    assert torch.equal(again["idx_out"], batch["idx_out"])
    after = buf.prio_leaf.cpu().numpy().view(np.uint32)
    p = ((out["td"].abs() + buf.eps) ** buf.alpha).cpu().numpy()
    q = quantise(p)
    want = before.copy()
    assert valid.sum() == 15 and float(out["td"][6]) == 0.0
    want[idx[valid]] = 0
    np.maximum.at(want, idx[valid], q[valid])
    np.testing.assert_array_equal(after, want)
    np.testing.assert_array_equal(after[idx[valid]], np.maximum(q[valid], want[idx[valid]]))
    assert (after[idx[valid]] != before[idx[valid]]).any()
