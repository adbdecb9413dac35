"""What wh_replay_prio_* refuse, against both libraries: the argument rules are csrc/abi_args.h's, so
the gfx950 library and the host engine return the same codes for the same calls (argument checks need
no device), and a refused or empty call touches nothing."""
import pytest

import prio_cases as pc


@pytest.fixture(scope="module")
def nat():
    from warehouse import _native

    return _native


def test_refusals_agree_between_the_libraries(nat):
    dev = pc.case_refusals(nat, nat.lib(), host=False)
    host = pc.case_refusals(nat, nat.host_lib(), host=True)
    assert dev == host


def test_new_symbols_are_declared_and_exported(nat):
    for name in ("wh_replay_prio_query", "wh_replay_prio_fill", "wh_replay_prio_update", "wh_replay_prio_sample"):
        assert name in nat.SYMBOLS
        assert hasattr(nat.lib(), name) and hasattr(nat.host_lib(), name)
