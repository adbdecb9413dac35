"""Cases of the policy network's action tail (emit_row, csrc/mlp_common.h), shared by
tests/test_gpu_policy_tail.py and its WH_MLP_LEGACY child process (this file run as a program).

Every check feeds the launch's OWN f32 logits (logits=True in the same launch) to the host model
(oracle/policy_tail.py), so the error of the logits never enters and what is compared is the tail alone:
the Philox words, the float32 uniform, the two logarithms and the first-maximum rule.

The sampler rule.  actions == model on every row whose model margin (the difference of the two largest
z_o - log(-log u_o)) exceeds MARGIN = 1e-3, and at most MAX_BELOW = 0.5 % of the rows may lie below it.
Where 1e-3 comes from: the device differs from the model only by taking the logarithm twice in fast
f32.  With a log good to a few ulp, -log u carries a relative error of order 2^-22, so log(-log u)
an absolute error of order 1e-6 plus a few ulp of a value below 18, again about 1e-6.  1e-3 is over a
hundred times that estimate; a disagreement above it is a finding about the kernel."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "rllib-warehouse_amd"), ROOT):      # (already there under pytest: tests/conftest.py)
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import policy_tail as pt  # noqa: E402

SEED = 0x9E3779B97F4A7C15          # both halves of the key non-zero
ROWS = 589                         # two full 256-row tasks + 77; four full 128-row f32 blocks + 77
STEPS = (0, 5, 0xFFFFFFFF)
SCALES = (1, 8, 100)               # of w2 and b2: logits of about +-0.3, +-3, +-40
MARGIN = 1e-3
MAX_BELOW = 0.005
KERNELS = [(v, p) for p in ("bf16", "f32") for v in ("small", "medium", "large")]


def scaled_net(wh, variant, precision, seed, scale):
    """MLPPolicy(variant, seed=seed) with w2 and b2 times `scale`, through the constructor's weights=."""
    net = wh.policy.MLPPolicy(variant, seed=seed, precision=precision)
    if scale == 1:
        return net
    w = dict(net.weights)
    w["w2"] = w["w2"] * np.float32(scale)
    w["b2"] = w["b2"] * np.float32(scale)
    return wh.policy.MLPPolicy(variant, weights=w, precision=precision)


def check_sampler(launch, seed, step, need_all_actions=False):
    """launch(**kw) -> (actions, logits) of one network on fixed rows.  One explore launch with logits,
    held to the model under the file's rule; the actions-only launch must give the same actions.
    Returns dict(rows, below: share of rows under MARGIN, worst: the largest model margin at which a
    row disagreed, 0.0 if none did, span: max |logit|)."""
    acts, lg = launch(explore=True, seed=seed, step=step, logits=True)
    acts, lg = acts.cpu().numpy(), lg.cpu().numpy()
    assert lg.dtype == np.float32 and np.isfinite(lg).all()
    assert ((0 <= acts) & (acts < 9)).all()
    want, margin, _ = pt.gumbel_actions(lg, seed, step)
    differ = acts != want
    worst = float(margin[differ].max()) if differ.any() else 0.0
    clear = margin > MARGIN
    stats = dict(rows=len(acts), below=float(1.0 - clear.mean()), worst=worst, span=float(np.abs(lg).max()))
    print("sampler", hex(seed), step, stats)
    assert stats["below"] <= MAX_BELOW, stats
    np.testing.assert_array_equal(acts[clear], want[clear], err_msg=f"sampler differs from the model: {stats}")
    if need_all_actions:
        assert len(np.unique(acts)) == 9, np.bincount(acts, minlength=9)
    only, none = launch(explore=True, seed=seed, step=step)
    assert none is None
    np.testing.assert_array_equal(only.cpu().numpy(), acts)
    return stats


def tie_patterns():
    """Nine b2 vectors as (b2, answer): for o = 0..7 the maximum stands at o and again at 8 with the
    other seven entries lower (all negative for odd o, so an argmax that starts from 0 instead of -inf
    fails too); then all nine equal, answer 0.  Every value is a small dyadic number."""
    out = []
    for o in range(8):
        lower = 0.5 - 0.0625 * ((np.arange(9) * 4) % 9)        # 0.5 .. 0.0, not monotone in the index
        b2 = lower.astype(np.float32)
        b2[[o, 8]] = 1.0
        if o % 2:
            b2 -= np.float32(2.0)
        out.append((b2, o))
    out.append((np.full(9, 0.75, np.float32), 0))
    return out


def check_b2_patterns(net, x):
    """w2 = 0, b2 = each pattern (repacked by load_weights from host arrays): the logits are exactly b2
    on every row (+0 * h sums to +0) and the argmax answers the FIRST maximum.  Returns the count."""
    base = dict(net.weights)
    n = 0
    for b2, answer in tie_patterns():
        net.load_weights(dict(base, w2=np.zeros_like(base["w2"]), b2=b2))
        acts, lg = net(x, logits=True)
        lg, acts = lg.cpu().numpy(), acts.cpu().numpy()
        assert (lg.view(np.uint32) == b2.view(np.uint32)[None, :]).all(), ("logits are not b2", b2, lg[0])
        assert (lg[:, answer] == lg.max(axis=1)).all() and (answer == 0 or (lg[:, 8] == lg[:, answer]).all())
        np.testing.assert_array_equal(acts, np.full(len(acts), answer), err_msg=f"b2 = {b2}")
        only, _ = net(x)
        np.testing.assert_array_equal(only.cpu().numpy(), acts)
        n += 1
    net.load_weights(base)
    return n


def random_rows(net, rows, seed):
    import torch

    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn((rows, net.in_dim), generator=g) * 4).to(net.device)


if __name__ == "__main__":   # the WH_MLP_LEGACY child of tests/test_gpu_policy_tail.py: Medium and Large on k_mlp
    import warehouse
    import warehouse.policy  # noqa: F401

    assert os.environ.get("WH_MLP_LEGACY") == "1"
    done = 0
    for variant in ("medium", "large"):
        net = scaled_net(warehouse, variant, "bf16", seed=31, scale=8)
        x = random_rows(net, ROWS, seed=6)
        check_sampler(lambda **kw: net(x, **kw), SEED, 5)
        done += 1 + check_b2_patterns(net, x)
    print("LEGACY TAIL OK", done)
