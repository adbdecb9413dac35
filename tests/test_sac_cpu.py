"""wh_sac_td without a GPU: the bodies of tests/sac_cases.py on the host engine (the same formula
header as the device kernel, a plain loop), the float32 transcription of the model, the Python
surface that needs no device, and the new kernels' resources.  (The refusal table is
tests/test_sac_refusals.py.)

The host engine and the float32 numpy model must stay under a QUARTER of the stated bounds on the
test's own inputs.  Largest errors seen, as fractions of the full bounds (y, td_rows, td): float32
model 0.046, 0.051, 0.0115; host engine 0.046, 0.051, 0.0107; on the peaked-policy case (logits up
to +-60, the bound formula with L = 60) float32 model 0.030, 0.022, 0.0053, host engine 0.033, 0.025,
0.0053."""
import os
import subprocess
import sys

import pytest

import sac_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nat():
    from warehouse import _native

    return _native


@pytest.mark.parametrize("M", sc.MS)
@pytest.mark.parametrize("NA", sc.NAS)
def test_td_on_the_host_engine_against_the_float64_model(nat, NA, M):
    worst = sc.case_td(nat, nat.host_lib(), "cpu", NA, M, quarter=True)
    print("host engine NA", NA, "M", M, "errors / bounds", worst)


@pytest.mark.parametrize("M", sc.MS)
@pytest.mark.parametrize("NA", sc.NAS)
def test_float32_model_stays_under_a_quarter_of_the_bounds(NA, M):
    worst = sc.case_float32_model(NA, M)
    print("float32 model NA", NA, "M", M, "errors / bounds", worst)


def test_agent_counts_reach_every_staging_head_and_both_td_sums():
    """The arithmetic behind sac_cases.NAS: which unaligned heads (floats up to the next 16-byte
    boundary) the blocks of k_sac_td meet at M = 300, from a 16-byte aligned array and from one 4 bytes
    off, and how many blocks there are."""
    heads, blocks = {}, {}
    for NA in sc.NAS:
        spw = sc.BLOCK_ROWS // NA
        blocks[NA] = -(-300 // spw)
        first = [b * spw * NA * 9 for b in range(blocks[NA])]        # a block's first float of a [rows, 9] array
        heads[NA] = [sorted({(4 - (f + off) % 4) % 4 for f in first}) for off in (0, 1)]
    assert all(blocks[NA] >= 4 for NA in sc.NAS if NA >= 3), blocks
    for NA in (1, 2, 4, 8, 9, 16):                                   # spans of whole 16-byte pieces: one head
        assert heads[NA] == [[0], [3]], (NA, heads[NA])
    for NA in (3, 5, 10, 11):                                        # the head changes from block to block
        assert len(heads[NA][0]) >= 2 and len(heads[NA][1]) >= 2, (NA, heads[NA])
    assert {h for NA in (3, 5, 10, 11) for hs in heads[NA] for h in hs} == {0, 1, 2, 3}
    assert [(sc.BLOCK_ROWS // NA) * NA * 9 % 4 for NA in (3, 5, 10, 11)] == [3, 3, 2, 1]
    assert {NA for NA in sc.NAS if 16 % NA == 0} == {1, 2, 4, 8, 16} and {3, 5, 9, 10, 11} <= set(sc.NAS)
    assert set(sc.MS) == {1, 65, 300}


def test_peaked_logits_are_what_the_case_states():
    import numpy as np

    pi = sc.peaked_logits(300, 7)
    assert pi.dtype == np.float32 and np.abs(pi).max() == sc.L_PEAKED
    assert (pi[0] == sc.L_PEAKED).all()                              # the row of nine equal logits
    rest = np.sort(pi[1:], axis=1)
    assert (rest[:, -1] == sc.L_PEAKED).all() and (rest[:, :-1] <= 0).all() and (rest[:, :-1] >= -sc.L_PEAKED).all()
    assert len(set(pi[1:].argmax(axis=1))) == 9
    assert (np.exp(np.float32(-120.0)) == 0) and (rest[:, -1] - rest[:, 0]).max() > 110     # exp underflows on some
    assert len([o for o in sc.OPTIONS if len(o) == 8 and o[7] == sc.L_PEAKED]) == 1


def test_model_on_a_hand_worked_row():
    """One row worked by hand: uniform policy, so p = 1/9 and logp = -ln 9 for every action."""
    import numpy as np

    inp = dict(pi_next=np.full((1, 9), 1.5, np.float32), q1t_next=np.arange(9, dtype=np.float32)[None],
               q2t_next=np.full((1, 9), 3.0, np.float32), q1=np.arange(9, dtype=np.float32)[None] * 2, q2=None,
               actions=np.array([[11]], np.int32), rewards=np.array([[1.0]], np.float32),
               dones=np.array([1], np.uint8), n=None)
    v = (0 + 1 + 2 + 3 * 6) / 9 + 0.5 * np.log(9.0)            # mean of min(q1t, 3) + alpha * ln 9
    y, td_rows, td = sc.model(inp, 1, alpha=0.5, discount=0.5, mask_dones=0)
    assert abs(y[0, 0] - (1 + 0.5 * v)) < 1e-12
    assert abs(td_rows[0, 0] - abs(8.0 - y[0, 0])) < 1e-12 and td[0] == td_rows[0, 0]   # action 11 -> 4: q1 = 8
    y, _, _ = sc.model(inp, 1, alpha=0.5, discount=0.5, mask_dones=1)
    assert y[0, 0] == 1.0


def test_python_surface_without_a_device():
    import warehouse
    import warehouse.policy as wp
    import warehouse.sac as ws

    assert "SACCritic" in warehouse.__all__ and "QNetwork" in warehouse.__all__
    assert ws.QNetwork is wp.MLPPolicy and warehouse.SACCritic is ws.SACCritic
    for name in ("load_weights", "copy_from"):
        assert callable(getattr(wp.MLPPolicy, name))
    import torch

    if not torch.cuda.is_available():   # no networks on the host engine: the constructor raises as MLPPolicy does
        with pytest.raises(RuntimeError, match="no HIP device"):
            wp.MLPPolicy("small")
        with pytest.raises(RuntimeError, match="no HIP device"):
            ws.QNetwork("small")


def test_weights_of_shares_the_modules_storage():
    import torch
    from warehouse.policy import weights_of

    net = torch.nn.Sequential(torch.nn.Linear(37, 256), torch.nn.ReLU(), torch.nn.Linear(256, 256), torch.nn.ReLU(),
                              torch.nn.Linear(256, 9))
    w = weights_of(net)
    assert sorted(w) == ["b0", "b1", "b2", "w0", "w1", "w2"]
    lin = [net[0], net[2], net[4]]
    for i, m in enumerate(lin):
        assert w[f"w{i}"].data_ptr() == m.weight.data_ptr() and w[f"b{i}"].data_ptr() == m.bias.data_ptr()
        assert not w[f"w{i}"].requires_grad and tuple(w[f"w{i}"].shape) == tuple(m.weight.shape)
    with pytest.raises(ValueError):
        weights_of(torch.nn.Sequential(torch.nn.Linear(3, 3), torch.nn.Tanh(), torch.nn.Linear(3, 3), torch.nn.ReLU(),
                                       torch.nn.Linear(3, 9)))


def test_new_kernels_have_no_scratch(nat):
    """tools/kernel_resources.py on the built library: k_sac_td and the eight k_mlp_pack instances,
    none with a private segment (scratch); k_sac_td's LDS is its five staged spans, the pack kernels
    use none."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources as kr
    finally:
        sys.path.pop(0)
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        ks = [k for co in kr.code_objects(nat.LIB_PATH, tmp) for k in kr.kernels(co)]
    names = subprocess.run(["c++filt"], input="\n".join(k["name"] for k in ks), capture_output=True, text=True).stdout
    sac = [k for k, d in zip(ks, names.splitlines()) if "k_sac_td" in d]
    pack = [k for k, d in zip(ks, names.splitlines()) if "k_mlp_pack" in d]
    assert len(sac) == 1 and len(pack) == 8
    assert sac[0]["scratch"] == 0 and sac[0]["lds"] <= 48 * 1024, sac[0]
    for k in pack:
        assert k["scratch"] == 0 and k["lds"] == 0, k
