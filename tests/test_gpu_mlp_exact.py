"""The policy MLP kernels against a float64 reference at tolerance 0, on the integer-valued networks of
tests/mlp_exact_cases.py (why exact answers exist, and the conditions tests/test_mlp_exact_cpu.py holds,
are written there).  Every comparison is np.array_equal on the logits as values (no NaN) and on the
actions, whose reference is the first maximum -- on the rows whose maximum is the planted tie of logits
2 and 6 too.

Routes: bf16 Small on k_mlp, Medium on k_mlp16 MODE 0, Large on k_mlp16 MODE 1, all three shapes on
k_mlp_f32, and Medium and Large on k_mlp in a WH_MLP_LEGACY=1 child process.  Entry points: forward
with logits, the actions-only launch, forward_x on the fragment image (bf16), forward_many with three
networks in one launch.  Packers: the host packer (the constructor) and wh_mlp_pack_device (load_weights
from device tensors), each held to the reference, so a map error both packers share shows here."""
import os
import subprocess
import sys

import pytest

import mlp_exact_cases as mx

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def wh():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    import warehouse
    import warehouse.policy  # noqa: F401

    return warehouse


@pytest.fixture(scope="module")
def nets(wh):
    """make_net(variant, precision, packer), built once per combination and shared."""
    cache = {}

    def get(variant, precision, packer):
        key = (variant, precision, packer)
        if key not in cache:
            cache[key] = mx.make_net(wh, variant, mx.SEED[variant], precision, packer)
        return cache[key]

    return get


@pytest.mark.parametrize("rows", mx.ROWS)
@pytest.mark.parametrize("precision", ["bf16", "f32"])
@pytest.mark.parametrize("variant", mx.VARIANTS)
def test_host_packed_network_is_exact(nets, variant, precision, rows):
    tied = mx.run_entry_points(nets(variant, precision, "host"), variant, rows, precision)
    assert rows < 300 or tied >= 20          # the planted tie is the maximum of that many rows


@pytest.mark.parametrize("rows", [33, 300])
@pytest.mark.parametrize("precision", ["bf16", "f32"])
@pytest.mark.parametrize("variant", mx.VARIANTS)
def test_device_packed_network_is_exact(nets, variant, precision, rows):
    import torch

    net = nets(variant, precision, "device")
    assert torch.equal(net.packed, nets(variant, precision, "host").packed)
    mx.run_entry_points(net, variant, rows, precision)


@pytest.mark.parametrize("precision", ["bf16", "f32"])
@pytest.mark.parametrize("variant", mx.VARIANTS)
def test_three_networks_in_one_launch_are_exact(wh, variant, precision):
    assert mx.run_many(wh, variant, precision) == 3


@pytest.mark.parametrize("variant", ["medium", "small"])
def test_persistent_walk_is_exact(wh, variant):
    import torch

    rows, compared = mx.run_walk(wh, variant)
    assert rows > 256 * torch.cuda.get_device_properties(0).multi_processor_count and compared >= 900


def test_legacy_route_is_exact_in_a_fresh_process():
    """bf16 Medium and Large with WH_MLP_LEGACY=1 (k_mlp on 32x32x16 tiles, MODE 0 and MODE 1): the
    choice is a process-wide static, so a fresh child process runs the 300-row case there."""
    env = dict(os.environ, WH_MLP_LEGACY="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mlp_exact_cases.py")], capture_output=True,
                       text=True, env=env, timeout=120)
    assert r.returncode == 0 and "LEGACY EXACT OK" in r.stdout, (r.stdout + r.stderr)[-3000:]
