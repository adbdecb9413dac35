"""The sync-free learner without a GPU: wh_adam_step_clock and wh_sac_td_la on the host engine (the bodies
of tests/sync_free_cases.py), their refusals on both libraries, the symbols, the new kernels' resources, and
the Python surface's ValueErrors that need no device.

Largest errors of wh_sac_td_la on the host engine seen at the three log_alphas, as fractions of the widened
bounds (y, td_rows, td): 0.060, 0.045, 0.0091.  Up to t = 2,000 at lr 1e-4 and 3e-4 the running-product table
never left adam_hyper's at all (0 f32 ulps, model and engine; the bound asserted is 1), and the engine's
clock equalled the Python model bit for bit."""
import ctypes
import os
import sys

import pytest

import adam_cases as ac
import sync_free_cases as sf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nat():
    from warehouse import _native

    return _native


# ----------------------------------------------------------------------------- the Adam clock
@pytest.mark.parametrize("lr", sf.LRS)
def test_running_products_stay_within_one_ulp_of_pow_in_the_model(nat, lr):
    print("model, lr", lr, "largest distance in f32 ulps", sf.case_model_against_pow(nat, lr))


@pytest.mark.parametrize("lr", sf.LRS)
def test_clock_on_the_host_engine_against_adam_hyper(nat, lr):
    sf.case_clock_against_pow(nat, nat.host_lib(), "cpu", lr)


@pytest.mark.parametrize("t0", (0, 1, 999))
def test_step_clock_is_adam_step_with_the_clocks_table(nat, t0):
    got = sf.case_step_is_adam_step_with_the_clocks_table(nat, nat.host_lib(), "cpu", t0)
    want = nat.adam_hyper(ac.LR, ac.BETAS[0], ac.BETAS[1], ac.EPS, t0 + 1)
    assert sf.ulps(sf.table(got.h), sf.table(want)).max() <= (0 if t0 == 0 else 1)


def test_clock_of_python_is_the_engines(nat):
    """_native.adam_clock(t) -- what DeviceAdam rebuilds from a checkpoint without products -- is the clock
    t ticks of the engine leave."""
    clock = sf.Clock(nat, "cpu")
    for _ in range(37):
        assert nat.host_lib().wh_adam_step_clock(0, None, clock.ptr, ac.LR, ac.BETAS[0], ac.BETAS[1], ac.EPS, None) == 0
    got, want = clock.read(), nat.adam_clock(37, *ac.BETAS)
    assert (got.t, got.beta1_t, got.beta2_t) == (want.t, want.beta1_t, want.beta2_t) and got.t == 37


# ----------------------------------------------------------------------------- TD targets, alpha read in place
@pytest.mark.parametrize("M", sf.TD_MS)
@pytest.mark.parametrize("NA", sf.TD_NAS)
def test_td_la_on_the_host_engine(nat, NA, M):
    print("host engine NA", NA, "M", M, "errors / bounds", sf.case_td_la(nat, nat.host_lib(), "cpu", NA, M))


def test_td_sizes_leave_a_partial_last_workgroup():
    assert all(256 // NA > 1 and 33 % (256 // NA) != 0 for NA in sf.TD_NAS) and sf.TD_MS == (1, 33)


# ----------------------------------------------------------------------------- refusals and symbols
def test_refusals_agree_between_the_libraries(nat):
    assert sf.case_clock_refusals(nat, nat.host_lib(), True) == sf.case_clock_refusals(nat, nat.lib(), False)
    assert sf.case_td_la_refusals(nat, nat.host_lib(), True) == sf.case_td_la_refusals(nat, nat.lib(), False)


def test_symbols_are_declared_bound_and_exported(nat):
    header = open(nat.HEADER).read()
    for s in ("wh_sac_td_la", "wh_adam_step_clock"):
        assert s in nat.SYMBOLS and f"int {s}(" in header
        for lib in (nat.lib(), nat.host_lib()):
            assert hasattr(lib, s) and getattr(lib, s).argtypes is not None and getattr(lib, s).restype is ctypes.c_int
    assert len(nat.lib().wh_sac_td_la.argtypes) == 5 and len(nat.lib().wh_adam_step_clock.argtypes) == 8
    C = nat.WhAdamClock      # wh_adam_clock as the header lays it out
    assert ctypes.sizeof(C) == 56 and ctypes.alignment(C) == 8
    assert {k: getattr(C, k).offset for k in ("t", "beta1_t", "beta2_t", "h")} == dict(t=0, beta1_t=8, beta2_t=16, h=24)
    assert "typedef struct wh_adam_clock" in header
    import warehouse

    assert {"SACLearner", "DeviceAdam", "CapturedUpdate"} <= set(warehouse.__all__)


def test_kernel_resources_are_the_recorded_ones(nat):
    """tools/kernel_resources.py on the built library: k_sac_td, k_adam and the three new kernels have the
    VGPRs, AGPRs, SGPRs, LDS and scratch of profiles/sync_free_kernel_resources.txt -- for k_sac_td and
    k_adam the lines recorded before the new kernels existed (76 / 63 and 41 / 38 registers); the kernel
    that reads log_alpha uses k_sac_td's LDS, the one that reads the clock and the tick none; none uses
    scratch."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources as kr
    finally:
        sys.path.pop(0)
    import subprocess
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        ks = [k for co in kr.code_objects(nat.LIB_PATH, tmp) for k in kr.kernels(co)]
    names = subprocess.run(["c++filt"], input="\n".join(k["name"] for k in ks), capture_output=True, text=True).stdout
    by = {}
    for k, d in zip(ks, names.splitlines()):
        for name in ("k_sac_td", "k_sac_la_td", "k_adam", "k_adam_clock", "k_adam_tick"):
            if f"::{name}(" in d:
                assert name not in by
                by[name] = k
    assert len(by) == 5, sorted(by)
    assert all(k["scratch"] == 0 for k in by.values()), by
    assert by["k_sac_la_td"]["lds"] == by["k_sac_td"]["lds"] <= 48 * 1024
    assert by["k_adam"]["lds"] == by["k_adam_clock"]["lds"] == by["k_adam_tick"]["lds"] == 0
    res = ("vgpr", "agpr", "sgpr", "lds", "scratch")
    recorded = {}
    for line in open(os.path.join(ROOT, "profiles", "sync_free_kernel_resources.txt")):
        f = line.split()
        if f and f[0] != "#":
            recorded[f[10].split("(")[0]] = tuple(int(f[i]) for i in (0, 2, 4, 6, 8))
    assert sorted(recorded) == sorted(by)
    for name, k in by.items():
        assert tuple(k[r] for r in res) == recorded[name], (name, k, recorded[name])
    assert recorded["k_sac_td"] == (76, 0, 63, 47184, 0) and recorded["k_adam"] == (41, 0, 38, 0, 0)
    for old, prof in (("k_sac_td", "sac_kernel_resources.txt"), ("k_adam", "sac_loss_kernel_resources.txt")):   # as first recorded
        first = [ln.split() for ln in open(os.path.join(ROOT, "profiles", prof)) if ln.split() and ln.split()[-1].startswith(old + "(")]
        assert len(first) == 1 and tuple(int(first[0][i]) for i in (0, 2, 4, 6, 8)) == recorded[old]


# ----------------------------------------------------------------------------- the Python surface
def test_capture_needs_sync_free():
    from warehouse import learner

    ln = learner.SACLearner.__new__(learner.SACLearner)
    ln.sync_free = False
    with pytest.raises(ValueError, match="sync_free"):
        ln.capture({})
    # with buf: it is the prioritized ring whose priorities the update sets, and the batch names its entries
    ln.sync_free = True

    class Ring:
        prioritized = False
    with pytest.raises(ValueError, match="prioritized"):
        ln.capture({"idx_out": None}, buf=Ring())
    Ring.prioritized = True
    with pytest.raises(ValueError, match="idx_out"):
        ln.capture({"obs": None}, buf=Ring())
    import torch

    with pytest.raises(ValueError, match="sync_free"):
        learner.SACLearner(None, None, None, rollout_policy=None, critic=None, log_alpha=torch.zeros(1), sync_free=1)


def test_replay_refuses_a_foreign_batch():
    import torch
    from warehouse import learner

    class NoGraph:
        def replay(self):
            raise AssertionError("a refused replay launched the graph")

    batch = dict(obs=torch.zeros(4, 3), actions=torch.zeros(4, dtype=torch.int32), weights=torch.ones(4))
    cap = learner.CapturedUpdate(None, NoGraph(), batch, {}, [])
    for bad in (dict(batch, obs=batch["obs"].clone()), dict(batch, extra=torch.zeros(1)),
                {k: v for k, v in batch.items() if k != "actions"}, {k: v for k, v in batch.items() if k != "weights"}):
        with pytest.raises(ValueError, match="captured"):
            cap.replay(bad)
    with pytest.raises(AssertionError):          # the captured tensors themselves pass the check
        cap.replay(dict(batch, weights=torch.full((4,), 0.5)))
    assert float(batch["weights"][0]) == 0.5     # ... and fresh weights are copied into the graph's own tensor


def test_critic_refuses_a_log_alpha_that_is_not_one_f32_element_on_its_device():
    import torch
    from warehouse import sac

    critic = sac.SACCritic.__new__(sac.SACCritic)
    critic.device = torch.device("cpu")
    for bad in (torch.zeros(2), torch.zeros(1, dtype=torch.float64), torch.zeros((), dtype=torch.int32), 0.0,
                torch.zeros(1, device="meta")):
        for fn in (critic.td, critic.targets):
            with pytest.raises(ValueError, match="log_alpha"):
                fn({}, log_alpha=bad)


def test_device_adam_takes_device_step_and_checkpoints_of_both_forms():
    import inspect
    from warehouse import learner

    p = inspect.signature(learner.DeviceAdam.__init__).parameters
    assert p["device_step"].default is False
    assert inspect.signature(learner.SACLearner.__init__).parameters["sync_free"].default is False
    assert isinstance(learner.DeviceAdam.t, property)
    a = learner.DeviceAdam([])                   # no tensors: no device needed
    a.step([])
    a.step([])
    assert a.t == 2 and a.state_dict()["step"] == 2 and "beta_t" not in a.state_dict()
    b = learner.DeviceAdam([])
    b.load_state_dict(dict(a.state_dict(), beta_t=(0.81, 0.998001)))      # the clock's products are the other form's
    assert b.t == 2
    with pytest.raises(ValueError, match="device_step"):
        learner.DeviceAdam([], device_step=True)
