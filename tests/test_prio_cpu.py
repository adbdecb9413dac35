"""The replay priority tree without a GPU: the bodies of tests/prio_cases.py on the host engine, the
Python surface, and the new kernels' resources.  (The refusal table is tests/test_prio_refusals.py.)"""
import os
import subprocess
import sys

import numpy as np
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


def test_levels_are_computed():
    """LEVELS against the hand count of the small trees and the entry counts of the deep ones."""
    assert [pc.LEVELS[c] for c in pc.COUNTS] == [1, 1, 2, 3, 4]
    assert [pc.LEVELS[c] for c in pc.DEEP_COUNTS + (pc.COUNT_7, pc.COUNT_8)] == [5, 5, 6, 7, 8]
    for c, lv in pc.LEVELS.items():
        levels = pc.shape(c)[2]
        assert len(levels) == lv and levels[-1][0] == 1 and (lv == 1 or levels[-2][0] > 1)
    assert [n for n, _ in pc.shape(65537)[2]] == [4097, 257, 17, 2, 1]            # the last leaf alone at every level
    assert pc.shape(1 << 20)[:2] == (1 << 20, sum(16 ** k for k in (4, 3, 2, 1)) + 16)   # no padding below the root


@pytest.mark.parametrize("count", (333, 4099))
def test_sparse_model_equals_the_dense_model(count):
    """SparseModel (the eight-level test's reference) against Model on the same fills, updates and
    draws: leaves, every level's non-zero entries, total, max_q and the samples."""
    d, s = pc.Model(count), pc.SparseModel(count)
    rng = np.random.default_rng(count)

    def same(what):
        leaf, node = d.arrays()
        parts = [leaf] + [node[off:off + n] for n, off in pc.shape(count)[2]]
        for k, part in enumerate(parts):
            idx, val = s.level(k)
            np.testing.assert_array_equal(np.flatnonzero(part), idx, err_msg=f"{what}: level {k}")
            np.testing.assert_array_equal(part[np.flatnonzero(part)].astype(np.uint64), val, err_msg=f"{what}: level {k}")
        assert d.total() == s.total() and d.max_q == s.max_q, what
        r = pc.philox_draws(pc.SEED, count, 300) + [0, pc.MASK64]
        for a, b in zip(d.sample(r), s.sample(r)):
            np.testing.assert_array_equal(a, b, err_msg=f"{what}: samples")

    def both(op, *args):
        getattr(d, op)(*args)
        getattr(s, op)(*args)
        same(f"{op}{args[:3] if op == 'fill' else (len(args[0]),)}")

    same("empty")
    idx = rng.integers(-2, count + 2, 40)
    idx[5] = idx[6] = idx[7]
    both("update", idx, rng.uniform(0.0, 30.0, 40).astype(np.float32))
    both("update", np.array([0, 15, 16, count - 1, -1, (1 << 31) + 5, 200, 200]), pc.QUANT_TABLE[:8])
    both("fill", 100, 150, 0, 777)
    both("fill", count - 30, 30, 0, pc.QMAX)
    both("fill", 120, 40, 0, 0)                                       # q = 0 removes leaves
    both("update", rng.integers(0, count, 200), rng.uniform(0.0, 4000.0, 200).astype(np.float32))
    both("fill", 3, count // 2, 1)
    assert d.max_q == pc.QMAX
    both("update", np.array([-1, count]), np.array([1.0, 2.0], np.float32))   # nothing valid
    both("fill", 0, count, 0, 0)
    assert s.total() == 0 and len(s.idx) == 0
    both("fill", 0, count, 0, pc.QMAX)


@pytest.mark.parametrize("count", pc.COUNTS + pc.DEEP_COUNTS)
def test_fills_and_updates_against_the_model(nat, count):
    pc.case_tree_ops(nat, nat.host_lib(), "cpu", count)


@pytest.mark.parametrize("count", pc.COUNTS + pc.DEEP_COUNTS)
def test_sampling_against_the_model(nat, count):
    pc.case_sampling(nat, nat.host_lib(), "cpu", count)


def test_seven_levels(nat):
    pc.case_seven_levels(nat, nat.host_lib(), "cpu")


def test_eight_levels_sparse(nat):
    pc.case_eight_levels_sparse(nat, nat.host_lib(), "cpu")


@pytest.mark.parametrize("count", (4099, 65537))
def test_wide_updates_and_samples(nat, count):
    pc.case_launch_widths(nat, nat.host_lib(), "cpu", count)


@pytest.mark.parametrize("count", (65537, (1 << 20) + 1))
def test_unaligned_fills_over_many_workgroups(nat, count):
    pc.case_unaligned_fills(nat, nat.host_lib(), "cpu", count)


@pytest.mark.parametrize("variant,na", [("medium", 8), ("small", 4)], ids=["medium8", "small4"])
def test_prioritized_buffer(variant, na):
    pc.case_buffer(make, variant, na)


def test_prioritized_buffer_of_five_levels():
    pc.case_buffer(make, "small", 4, **pc.BIG)


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
