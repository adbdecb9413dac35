"""What wh_adam_step refuses, against both libraries (wh_abi::adam_call of csrc/abi_args.h: identical codes,
nothing touched by a refused or empty call), and the ValueErrors of warehouse.DeviceAdam."""
import pytest

import adam_cases as ac


@pytest.fixture(scope="module")
def nat():
    from warehouse import _native

    return _native


def test_refusals_agree_between_the_libraries(nat):
    dev = ac.case_refusals(nat, nat.lib(), host=False)
    host = ac.case_refusals(nat, nat.host_lib(), host=True)
    assert dev == host


def test_new_symbol_is_declared_bound_and_exported(nat):
    import ctypes

    assert "wh_adam_step" in nat.SYMBOLS and nat.WH_ADAM_MAX_SEGS == 24
    for L in (nat.lib(), nat.host_lib()):
        assert hasattr(L, "wh_adam_step") and L.wh_adam_step.restype is ctypes.c_int and L.wh_adam_step.argtypes
    header = open(nat.HEADER).read()
    assert "#define WH_ADAM_MAX_SEGS 24" in header
    assert ctypes.sizeof(nat.WhAdamSeg) == 40 and ctypes.sizeof(nat.WhAdamHyper) == 28


def test_device_adam_value_errors():
    import torch
    import warehouse

    with pytest.raises(ValueError, match="24"):
        warehouse.DeviceAdam([torch.zeros(3) for _ in range(25)])
    for bad in ([torch.zeros(3, dtype=torch.float64)], [torch.zeros(4, 4).t()], [torch.zeros(3), None],
                [torch.zeros(3), torch.zeros(3, device="meta")]):
        with pytest.raises(ValueError):
            warehouse.DeviceAdam(bad)
