"""bench.py on the GPU: a plain run measures the headline alone, --steps sets the timed steps, and
--dump-outputs writes what the timed path computed in its last step -- checked against the oracle
run for the same number of steps (bit-exact, as everywhere: integer state, rewards sums of 1.0f)."""
import json
import os
import sys

import numpy as np
import pytest

from oracle import batched as ob
from oracle import core as oc

pytestmark = pytest.mark.gpu

B, NA, K, W, SEED = 96, 8, 45, 7, 1234        # bench.py's own seed; K and W no multiples of --chunk 20
FULL_ONLY = ("alt_launch_mode", "desync_episodes", "sampler_path", "sampler_path_c4", "sampler_fragments",
             "vector_path", "vector_path_large_train", "vector_path_dict_order", "policy_path", "policy_path_f32")


@pytest.fixture(scope="module")
def oracle_steps():
    """n -> (rewards, dones of step n, state after it) of the oracle's greedy rollout with auto-reset
    from the reset state; shared by the cases (both modes end on the same step)."""
    L = oc.layout_for("medium")
    cache = {}

    def at(n):
        if n not in cache:
            S = ob.BState.zeros(L, B, NA)
            d = ob.PhiloxDraws(SEED, np.arange(B))
            ob.reset(L, S, d)
            for _ in range(n):
                rew, done, _, _ = ob.step(L, S, ob.greedy(L, S, 0.0, d), d)
                if done.any():
                    ob.reset(L, S, d, mask=done)
            cache[n] = (rew, done, S)
        return cache[n]

    return at


@pytest.mark.parametrize("mode", ["graph", "fused"])
def test_plain_run_dumps_the_last_timed_step(mode, tmp_path, monkeypatch, capsys, oracle_steps):
    import bench

    out = str(tmp_path / "dump")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", str(K), "--warmup", str(W), "--envs", str(B),
                                      "--chunk", "20", "--mode", mode, "--dump-outputs", out])
    for k in bench.KERNEL_OVERRIDES + ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == K and line["warmup"] == W and line["full"] is False
    assert line["ms_per_step"] == pytest.approx(line["window"]["union_s"] * 1e3 / K)
    assert line["value"] == pytest.approx(B * NA * K / line["window"]["union_s"])
    assert line["roofline"]["launches"] == (K if mode == "graph" else 3)          # 20 + 20 + 5 steps
    # a plain run measures nothing but the headline
    assert all(line[k] is None for k in FULL_ONLY) and line["config_legs"] == {}
    assert "cpu_baseline" not in line and "gpu_over_cpu" not in line
    # the env has taken setup_steps + W + K steps since its reset when the window closes
    n = line["config"]["window"]["setup_steps"] + W + K
    rew, done, S = oracle_steps(n)
    got = {f[:-4]: np.load(os.path.join(out, f)) for f in sorted(os.listdir(out))}
    assert set(got) == {"rewards", "dones"} | {"state_" + k for k in ("pos", "agent_target", "pickup_target",
                                                                      "pickup_timer", "t", "n", "fresh", "episode")}
    assert all(a.dtype == np.float32 and a.shape[0] == B for a in got.values())
    np.testing.assert_array_equal(got["rewards"], rew)
    np.testing.assert_array_equal(got["dones"], done.astype(np.float32))
    for name, field in (("pos", S.pos), ("agent_target", S.agent_tgt), ("pickup_target", S.pk_tgt),
                        ("pickup_timer", S.pk_timer), ("t", S.t), ("n", S.n), ("fresh", S.fresh),
                        ("episode", S.episode)):
        np.testing.assert_array_equal(got["state_" + name], field.astype(np.float32), err_msg=name)
    assert line["config"]["window"]["dones_in_window"] == (None if mode == "graph" else B)   # one episode end
