"""The refusal table of wh_replay_record against both libraries (argument checks need no device):
the same calls, the same codes; refused and empty calls touch nothing."""


def test_refusals_agree_between_the_libraries():
    from warehouse import _native as nat

    import record_cases as rec

    dev = rec.case_refusals(nat, nat.lib(), host=False)
    host = rec.case_refusals(nat, nat.host_lib(), host=True)
    assert dev == host and len(dev) >= 25
