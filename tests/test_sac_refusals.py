"""What wh_sac_td refuses, against both libraries: the argument rules are csrc/abi_args.h's, so the
gfx950 library and the host engine return the same codes for the same calls (argument checks need no
device), and a refused or empty call touches nothing.  wh_mlp_pack_device is device only: the host
engine exports it and answers WH_ENOTSUP like its other wh_mlp_* entry points."""
import ctypes

import pytest

import sac_cases as sc


@pytest.fixture(scope="module")
def nat():
    from warehouse import _native

    return _native


def test_refusals_agree_between_the_libraries(nat):
    dev = sc.case_refusals(nat, nat.lib(), host=False)
    host = sc.case_refusals(nat, nat.host_lib(), host=True)
    assert dev == host


def test_new_symbols_are_declared_and_exported(nat):
    for name in ("wh_mlp_pack_device", "wh_sac_td"):
        assert name in nat.SYMBOLS
        assert hasattr(nat.lib(), name) and hasattr(nat.host_lib(), name)


def test_pack_device_is_not_supported_on_the_host_engine(nat):
    import torch

    desc = nat.WhMlpDesc(37, 256, 256, 9, nat.WH_MLP_BF16)
    bufs = [torch.full((64,), 0xA5, dtype=torch.uint8) for _ in range(7)]
    rc = nat.host_lib().wh_mlp_pack_device(ctypes.byref(desc), *[b.data_ptr() for b in bufs], None)
    assert rc == nat.WH_ENOTSUP
    assert all(bool((b == 0xA5).all()) for b in bufs)


def test_pack_device_argument_refusals_need_no_device(nat):
    """The device library's own refusals come before anything touches the GPU: d == NULL and every
    NULL pointer WH_EINVAL, a misaligned blob WH_EINVAL, an unknown shape WH_ENOTSUP."""
    lib = nat.lib()
    desc = nat.WhMlpDesc(37, 256, 256, 9, nat.WH_MLP_BF16)
    ptrs = [4096 * (i + 1) for i in range(7)]          # dummies: a refused call dereferences nothing
    assert lib.wh_mlp_pack_device(None, *ptrs, None) == nat.WH_EINVAL
    for i in range(7):
        p = list(ptrs)
        p[i] = None
        assert lib.wh_mlp_pack_device(ctypes.byref(desc), *p, None) == nat.WH_EINVAL, i
    for off in (4, 8, 1):
        assert lib.wh_mlp_pack_device(ctypes.byref(desc), *ptrs[:6], ptrs[6] + off, None) == nat.WH_EINVAL, off
    for bad in (nat.WhMlpDesc(38, 256, 256, 9, nat.WH_MLP_BF16), nat.WhMlpDesc(37, 256, 256, 8, nat.WH_MLP_BF16),
                nat.WhMlpDesc(37, 256, 256, 9, 7), nat.WhMlpDesc(82, 512, 256, 9, nat.WH_MLP_F32)):
        assert lib.wh_mlp_pack_device(ctypes.byref(bad), *ptrs, None) == nat.WH_ENOTSUP
