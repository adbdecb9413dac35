"""The multi-network MLP launch without a device: the built library holds one GridMulti kernel beside
each of the eight one-network kernels, with the same LDS and no more scratch (tools/kernel_resources.py
reads the code object's metadata), and the Python surface -- forward_many, SACCritic(fused=...) --
exists and refuses what it must before anything reaches the GPU."""
import importlib.util
import os
import re
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mlp_kernels():
    from warehouse import _native

    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    with tempfile.TemporaryDirectory() as tmp:
        ks = [k for co in kr.code_objects(_native.LIB_PATH, tmp) for k in kr.kernels(co)]
    for k, d in zip(ks, kr.demangle([k["name"] for k in ks])):
        k["demangled"] = d
    out = {}
    for k in ks:
        m = re.search(r"::(k_mlp16|k_mlp_f32|k_mlp)<\(anonymous namespace\)::(Net\w*<[^>]*>), \(anonymous namespace\)::(Grid\w+)>",
                      k["demangled"])
        if m:
            out[(m.group(1), m.group(2), m.group(3))] = k
    return out


def test_eight_multi_kernels_within_their_one_network_kernels_resources(mlp_kernels):
    multi = {k[:2]: v for k, v in mlp_kernels.items() if k[2] == "GridMulti"}
    one = {k[:2]: v for k, v in mlp_kernels.items() if k[2] == "GridOne"}
    assert len(multi) == 8 and set(multi) == set(one), sorted(mlp_kernels)
    # the registered shapes: k_mlp16 Medium / Large, k_mlp Small / Medium / Large, k_mlp_f32 all three
    assert sorted(k for k, _ in multi) == ["k_mlp"] * 3 + ["k_mlp16"] * 2 + ["k_mlp_f32"] * 3
    for key, m in multi.items():
        o = one[key]
        assert m["lds"] == o["lds"], (key, m, o)
        assert m["scratch"] <= o["scratch"], (key, m, o)
        # bf16: two waves per SIMD need <= 256 registers; f32: one (<= 512 with the AGPRs)
        assert m["vgpr"] <= o["vgpr"] and m["agpr"] <= o["agpr"], (key, m, o)


def test_forward_many_and_fused_exist_and_refuse_without_a_device():
    import torch
    import warehouse
    import warehouse.policy as wp
    from warehouse import sac

    assert warehouse.forward_many is wp.forward_many and "forward_many" in warehouse.__all__
    assert wp.MAX_JOBS == 8
    assert wp.forward_many([]) == []
    with pytest.raises(ValueError, match="at most 8"):
        wp.forward_many([{}] * 9)
    with pytest.raises(ValueError, match="MLPPolicy"):
        wp.forward_many([dict(net=object(), obs=torch.zeros(3, 37))])
    with pytest.raises(ValueError, match="unknown job keys"):
        wp.forward_many([dict(network=None)])
    import inspect

    assert inspect.signature(sac.SACCritic.__init__).parameters["fused"].default is None
    assert isinstance(sac.FUSED_MAX_ROWS, int) and sac.FUSED_MAX_ROWS > 0
    with pytest.raises(ValueError, match="MLPPolicy"):
        sac.SACCritic(object(), object(), None, object(), None, alpha=0.2, fused=True)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):     # as MLPPolicy itself: device only
            wp.MLPPolicy("small")
