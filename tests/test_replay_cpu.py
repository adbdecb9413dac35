"""The replay ring without a GPU: the bodies of tests/replay_cases.py on the host engine, the
refusal table against both libraries (argument checks need no device), the Python surface, and the
new kernels' resources."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import replay_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make(variant, num_envs, num_agents, **kw):
    import warehouse

    return warehouse.BatchedWarehouse(variant, num_envs, num_agents, device="cpu", **kw)


@pytest.fixture(scope="module")
def nat():
    from warehouse import _native

    return _native


@pytest.mark.parametrize("variant,na,train", rc.VARIANTS, ids=rc.IDS)
def test_round_trip_against_the_oracle(variant, na, train):
    rc.case_round_trip(make, variant, na, train)


@pytest.mark.parametrize("full", [True, False], ids=["full", "sparse"])
@pytest.mark.parametrize("variant,na,train", rc.VARIANTS, ids=rc.IDS)
def test_round_trip_from_fuzzed_states(variant, na, train, full):
    rc.case_round_trip_fuzzed(make, variant, na, train, full)


@pytest.mark.parametrize("variant,na,train", [("medium", 8, False), ("medium", None, True)], ids=["medium8", "medium_train"])
def test_step_leaves_the_trajectory_alone(variant, na, train):
    rc.case_step_keeps_trajectory(make, variant, na, train)


def test_index_draw():
    rc.case_index_draw(make)


@pytest.mark.parametrize("variant,na,train", [("medium", 8, False), ("medium", 3, False), ("large", 16, False)],
                         ids=["medium8", "medium3", "large16"])
def test_invalid_indices(variant, na, train):
    rc.case_invalid_indices(make, variant, na, train)


def test_refusals_agree_between_the_libraries(nat):
    """The same calls, the same codes from both libraries; refused calls touch nothing."""
    dev = rc.case_refusals(nat, nat.lib(), host=False)
    host = rc.case_refusals(nat, nat.host_lib(), host=True)
    assert dev == host


def test_host_engine_has_no_fragments(nat):
    """A fragment output is WH_ENOTSUP on the host engine (after the argument checks), and
    ReplayBuffer.sample(fragments=True) raises instead of returning rows."""
    env = make("small", 4, 4)
    env.reset()
    import warehouse

    buf = warehouse.ReplayBuffer(env, 2)
    buf.step(env.policy())
    frag = torch.zeros(4096, dtype=torch.uint8)
    n = torch.zeros(3, dtype=torch.int32)
    batch = nat.WhReplayBatch(xfrag=frag.data_ptr(), n=n.data_ptr())
    call = lambda b, filled=1: nat.host_lib().wh_replay_gather(   # noqa: E731
        env._cfgp, env.B, ctypes.byref(buf._ring), filled, 3, None, 0, 0, ctypes.byref(b), None)
    assert call(batch) == nat.WH_ENOTSUP
    assert call(batch, filled=3) == nat.WH_EINVAL            # the argument checks come first
    assert not frag.any() and not n.any()
    with pytest.raises(nat.WarehouseNativeError, match="fragment"):
        buf.sample(3, fragments=True)


def test_python_surface():
    import warehouse

    assert "ReplayBuffer" in warehouse.__all__
    env = make("medium", 5, 2, seed=3)
    env.reset()
    with pytest.raises(ValueError):
        warehouse.ReplayBuffer(env, 0)
    buf = warehouse.ReplayBuffer(env, 3)
    assert (buf.filled, buf.cursor, len(buf)) == (0, 0, 0)
    with pytest.raises(ValueError, match="no transition"):
        buf.sample(4)
    for s in range(4):
        obs, rew, done = buf.step(env.policy("greedy", 0.1))
        assert obs is env._obs and rew is env.rewards and done is env.dones
    assert (buf.filled, buf.cursor, len(buf)) == (3, 1, 15)
    assert buf.step(env.policy(), observe=False)[0] is None
    a = buf.sample(6)
    assert set(a) == {"obs", "next_obs", "actions", "rewards", "dones", "n", "idx_out"}
    assert a["obs"].shape == (6, 2, 82) and a["idx_out"].dtype == torch.int64
    b = buf.sample(6, rows=False, states=True)
    assert set(b) == {"state", "next_state", "actions", "rewards", "dones", "n", "idx_out"}
    assert b["actions"] is a["actions"]                       # buffer-owned, overwritten by the next call
    assert buf.sample(0)["n"].shape == (0,)
    with pytest.raises(ValueError):
        buf.sample(2, idx=[1, 2, 3])
    with pytest.raises(ValueError):
        buf.sample(2, out=dict(obs=torch.zeros((2, 2, 81))))
    with pytest.raises(ValueError):
        buf.put_obs(3)
    buf.put_obs(1)                                            # env.actions by default
    buf.put_next(1)
    got = buf.sample(5, idx=np.arange(5) + 5, states=True)
    assert torch.equal(got["state"], env.state) and torch.equal(got["next_state"], env.state)
    assert torch.equal(got["actions"], env.actions)


def test_replay_kernels_keep_their_registers(nat):
    """tools/kernel_resources.py on the built library: one put and three gather instances per
    registry entry, none with a private segment (scratch), LDS within a workgroup's 64 KB."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources as kr
    finally:
        sys.path.pop(0)
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        ks = kr.kernels(kr.code_object(nat.LIB_PATH, tmp))
    names = subprocess.run(["c++filt"], input="\n".join(k["name"] for k in ks), capture_output=True, text=True).stdout
    mine = [(k, d) for k, d in zip(ks, names.splitlines()) if "k_replay_" in d]
    assert sum("k_replay_put" in d for _, d in mine) == 10 and sum("k_replay_gather" in d for _, d in mine) == 30
    for k, _ in mine:
        assert k["scratch"] == 0 and k["lds"] <= 64 * 1024, k
