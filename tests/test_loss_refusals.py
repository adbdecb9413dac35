"""What wh_sac_loss and wh_sac_loss_query refuse, against both libraries: the argument rules are
csrc/abi_args.h's (wh_abi::sac_loss_call), so the gfx950 library and the host engine return the same codes
for the same calls (argument checks need no device), and a refused or empty call touches nothing.  Then the
ValueErrors of warehouse.sac_losses, which come before any native call."""
import pytest

import loss_cases as lc


@pytest.fixture(scope="module")
def nat():
    from warehouse import _native

    return _native


def test_refusals_agree_between_the_libraries(nat):
    dev = lc.case_refusals(nat, nat.lib(), host=False)
    host = lc.case_refusals(nat, nat.host_lib(), host=True)
    assert dev == host


def test_new_symbols_are_declared_bound_and_exported(nat):
    import ctypes

    for name in ("wh_sac_loss", "wh_sac_loss_query"):
        assert name in nat.SYMBOLS
        for L in (nat.lib(), nat.host_lib()):
            assert hasattr(L, name) and getattr(L, name).restype is ctypes.c_int and getattr(L, name).argtypes
    header = open(nat.HEADER).read()
    assert "SAC LOSSES" in header and header.index("SAC TD TARGETS") < header.index("SAC LOSSES")
    assert ctypes.sizeof(nat.WhSacLossArgs) == 8 * 8 + 2 * 4 + 5 * 8


def test_sac_losses_value_errors_come_before_any_native_call():
    import torch
    import warehouse

    M, NA = 3, 4
    good = dict(pi=torch.zeros(M * NA, 9), q1=torch.zeros(M * NA, 9), q2=torch.zeros(M * NA, 9), y=torch.zeros(M, NA),
                actions=torch.zeros(M, NA, dtype=torch.int32))
    kw = dict(log_alpha=torch.zeros(1), target_entropy=0.935)

    def call(over=None, **extra):
        a = dict(good, **(over or {}))
        return warehouse.sac_losses(a["pi"], a["q1"], a["q2"], a["y"], a["actions"], **dict(kw, **extra))

    for over in (dict(pi=torch.zeros(M * NA, 8)), dict(pi=torch.zeros(M * NA + 1, 9)), dict(q1=torch.zeros(M * NA, 9).double()),
                 dict(q2=torch.zeros(9, M * NA).t()), dict(y=torch.zeros(M * NA)), dict(y=torch.zeros(M, 17)),
                 dict(actions=torch.zeros(M, NA, dtype=torch.int64)), dict(pi=None)):
        with pytest.raises(ValueError):
            call(over)
    for extra in (dict(n=torch.zeros(M, dtype=torch.int64)), dict(n=torch.zeros(M + 1, dtype=torch.int32)),
                  dict(weights=torch.zeros(M, NA)), dict(log_alpha=torch.zeros(2)), dict(log_alpha=0.0),
                  dict(out=dict(td=torch.zeros(M))), dict(out=dict(stats=torch.zeros(5))),
                  dict(out=dict(dpi=torch.zeros(M * NA, 9, dtype=torch.float64)))):
        with pytest.raises(ValueError):
            call(**extra)
    with pytest.raises(ValueError):                      # dq2 is no output without q2
        call(dict(q2=None), out=dict(dq2=torch.zeros(M * NA, 9)))
    assert {"SACLearner", "DeviceAdam", "sac_losses"} <= set(warehouse.__all__)
