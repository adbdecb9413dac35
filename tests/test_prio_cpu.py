"""The replay priority tree without a GPU: the bodies of tests/prio_cases.py on the host engine, the
Python surface, and the new kernels' resources.  (The refusal table is tests/test_prio_refusals.py.)"""
import os
import subprocess
import sys

import pytest

import prio_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make(variant, num_envs, num_agents, **kw):
    import warehouse

    return warehouse.BatchedWarehouse(variant, num_envs, num_agents, device="cpu", **kw)


@pytest.fixture(scope="module")
def nat():
    from warehouse import _native

    return _native


def test_quantisation_table_of_the_model():
    pc.case_quantisation_model()


@pytest.mark.parametrize("count", pc.COUNTS)
def test_fills_and_updates_against_the_model(nat, count):
    pc.case_tree_ops(nat, nat.host_lib(), "cpu", count)


@pytest.mark.parametrize("count", pc.COUNTS)
def test_sampling_against_the_model(nat, count):
    pc.case_sampling(nat, nat.host_lib(), "cpu", count)


@pytest.mark.parametrize("variant,na", [("medium", 8), ("small", 4)], ids=["medium8", "small4"])
def test_prioritized_buffer(variant, na):
    pc.case_buffer(make, variant, na)


def test_plain_buffer_has_no_tree():
    pc.case_plain_buffer(make)


def test_prio_kernels_have_no_scratch(nat):
    """tools/kernel_resources.py on the built library: the three kernels, none with a private
    segment (scratch), LDS of a few words."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources as kr
    finally:
        sys.path.pop(0)
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        ks = kr.kernels(kr.code_object(nat.LIB_PATH, tmp))
    names = subprocess.run(["c++filt"], input="\n".join(k["name"] for k in ks), capture_output=True, text=True).stdout
    mine = {d.split("::")[1].split("(")[0]: k for k, d in zip(ks, names.splitlines()) if "k_prio_" in d}
    assert sorted(mine) == ["k_prio_fill", "k_prio_sample", "k_prio_update"]
    for k in mine.values():
        assert k["scratch"] == 0 and k["lds"] <= 256, k
