"""The two libraries behind include/warehouse_amd.h refuse the same calls: one table of calls to
every step-family entry point and to wh_pack / wh_unpack / wh_reset / wh_observe(_x), with the return
code the header's contract gives, run against the gfx950 library and the host engine.  The argument
rules are written once (csrc/abi_args.h), so both answer alike; the host engine answers WH_ENOTSUP
for the entries it does not implement.

No call gets as far as a launch: a batch of B > 0 envs appears only where the call is refused on
the host side first (its pointers are never dereferenced), every call that is accepted is an empty
batch.  So the table runs the same with or without a GPU.

Rows that fit only one of the pack / reset / observe entries, and the one config on which the two
libraries answer differently (racks that overlap), are in ENTRY_ROWS below the table."""
import ctypes

import pytest

from warehouse import _native as nat

OK, EINVAL, ENOTSUP = nat.WH_OK, nat.WH_EINVAL, nat.WH_ENOTSUP

# argument names of every entry point of the table, in the header's order
_ROLLOUT = ("cfg B state steps policy p rewards dones returns stats autoreset variable_n seed env_offset")
ENTRIES = {
    "wh_step": "cfg B state actions order order_len rewards dones regen n_inactive phase seed env_offset stream",
    "wh_policy": "cfg B state policy p actions seed env_offset stream",
    "wh_rollout": _ROLLOUT + " stream",
    "wh_rollout_prepare": _ROLLOUT + " stream out",
    "wh_vector_step": "cfg B state actions order order_len mask rewards dones obs stats autoreset variable_n "
                      "seed env_offset stream",
    "wh_vector_step_x": "cfg B state actions order order_len mask rewards dones xfrag stats autoreset variable_n "
                        "seed env_offset stream",
    "wh_sampler_step": "cfg B state policy p rewards dones obs stats variable_n seed env_offset stream",
    "wh_sampler_rollout": "cfg B state steps policy p rewards dones obs stats variable_n seed env_offset stream",
    "wh_sampler_step_to": "cfg B state state_out policy p rewards dones stats variable_n seed env_offset stream",
    "wh_step_wide": "cfg B state actions rewards dones regen n_inactive seed env_offset lanes stream",
    "wh_rollout_wide": _ROLLOUT + " lanes stream",
    "wh_vector_step_wide": "cfg B state actions mask rewards dones obs stats autoreset variable_n seed env_offset "
                           "lanes stream",
    "wh_pack": "cfg B pos agent_target pickup_target pickup_timer t n fresh episode state stream",
    "wh_unpack": "cfg B state pos agent_target pickup_target pickup_timer t n fresh episode stream",
    "wh_reset": "cfg B state mask draws variable_n seed env_offset stream",
    "wh_observe": "cfg B state rows stream",
    "wh_observe_x": "cfg B state rows xrows stream",
}
ENTRIES = {k: tuple(v.split()) for k, v in ENTRIES.items()}
# device-only entries: the host engine answers WH_ENOTSUP whatever the arguments
HOST_ENOTSUP = {"wh_rollout_prepare", "wh_vector_step_x", "wh_sampler_step_to", "wh_step_wide", "wh_rollout_wide",
                "wh_vector_step_wide", "wh_observe_x"}
# (wh_observe's rows are "rows" / "xrows" here: the table's obs and xfrag rows state the step family's
# rules -- obs optional, xfrag required and checked for an empty batch too -- which are not wh_observe_x's)
CANONICAL = ("pos", "agent_target", "pickup_target", "pickup_timer", "t", "n", "fresh", "episode")
POINTERS = {"state", "actions", "order", "mask", "rewards", "dones", "returns", "regen", "n_inactive", "obs", "xfrag",
            "state_out", "rows", "xrows", *CANONICAL}
DUMMY = 4096   # a 16-byte aligned address that a refused call never dereferences
NA = 4         # agent slots of the base config (Small)


def config(**over):
    """WarehouseSmall with 4 agents (variants.py:19-32), fields replaced by `over`."""
    f = dict(area_dimension=12, num_requests=4, racks=(4, 8), agent_slots=NA, episode_duration=200,
             pickup_wait_duration=200)
    num_racks = over.pop("num_racks", None)
    f.update(over)
    cfg = nat.make_config(f["area_dimension"], f["num_requests"], f["racks"], f["agent_slots"],
                          f["episode_duration"], f["pickup_wait_duration"])
    if num_racks is not None:
        cfg.num_racks = num_racks
    return cfg


def bins_only():
    """Episode bins without the per-env return accumulator they are folded from."""
    return nat.WhEpisodeStats(None, DUMMY, None, None, None)


# ---- the table: (what is wrong, the arguments that make it so, the code).  A row applies to every
# entry point that takes all of the named arguments ("cfg" rows: to all).  ANY rows are refused
# whatever the batch, so they run with B = 0 and with B = 8 over dummy pointers, and with steps = 0
# where the entry takes steps.  BATCH rows are refused only for B > 0 (and steps > 0 if they name
# steps): the same call with B = 0 or steps = 0 is the valid empty batch, WH_OK.
ANY, BATCH = "any", "batch"
TABLE = [
    ("null config", dict(cfg=None), EINVAL, ANY),
    ("no racks", dict(cfg=config(num_racks=0)), EINVAL, ANY),
    ("too many racks", dict(cfg=config(num_racks=nat.WH_MAX_RACKS + 1)), EINVAL, ANY),
    ("area too small", dict(cfg=config(area_dimension=4)), EINVAL, ANY),
    ("area too large", dict(cfg=config(area_dimension=33)), EINVAL, ANY),
    ("no agent slots", dict(cfg=config(agent_slots=0)), EINVAL, ANY),
    ("more agent slots than requests", dict(cfg=config(agent_slots=5)), EINVAL, ANY),
    ("more requests than pickup points", dict(cfg=config(num_requests=17)), EINVAL, ANY),
    ("more requests than delivery points", dict(cfg=config(area_dimension=6, racks=(2, 4), num_requests=9)), EINVAL, ANY),
    ("zero pickup wait", dict(cfg=config(pickup_wait_duration=0)), EINVAL, ANY),
    ("pickup wait past the 8-bit timer", dict(cfg=config(pickup_wait_duration=256)), EINVAL, ANY),
    ("negative episode duration", dict(cfg=config(episode_duration=-1)), EINVAL, ANY),
    ("rack on the low border", dict(cfg=config(racks=(1, 8))), ENOTSUP, ANY),
    ("rack on the high border", dict(cfg=config(racks=(4, 11))), ENOTSUP, ANY),
    ("B < 0", dict(B=-1), EINVAL, ANY),
    ("B < 0, no pointers", dict(B=-5, state=None), EINVAL, ANY),
    ("policy 0", dict(policy=0), EINVAL, ANY),
    ("policy 3", dict(policy=3), EINVAL, ANY),
    ("policy 7", dict(policy=7), EINVAL, ANY),
    ("p < 0", dict(p=-0.1), EINVAL, ANY),
    ("p > 1", dict(p=1.5), EINVAL, ANY),
    ("p NaN", dict(p=float("nan")), EINVAL, ANY),
    ("steps < 0", dict(steps=-1), EINVAL, ANY),
    ("bins without episode_return", dict(stats=bins_only()), EINVAL, ANY),
    ("phase below range", dict(phase=-1), EINVAL, ANY),
    ("phase above range", dict(phase=3), EINVAL, ANY),
    ("order width 4 NA + 1", dict(order_len=4 * NA + 1), EINVAL, ANY),
    ("order width < 0", dict(order_len=-1), EINVAL, ANY),
    ("lanes 0", dict(lanes=0), EINVAL, ANY),
    ("lanes 2", dict(lanes=2), EINVAL, ANY),
    ("lanes 8", dict(lanes=8), EINVAL, ANY),
    ("lanes 32", dict(lanes=32), EINVAL, ANY),
    ("lanes 64", dict(lanes=64), EINVAL, ANY),
    ("lanes < 0", dict(lanes=-16), EINVAL, ANY),
    ("misaligned xfrag", dict(xfrag=DUMMY + 4), EINVAL, ANY),
    ("no handle out", dict(out=None), EINVAL, ANY),
    ("missing state", dict(state=None), EINVAL, BATCH),
    ("missing actions", dict(actions=None), EINVAL, BATCH),
    ("missing obs", dict(obs=None, steps=3), EINVAL, BATCH),   # (only wh_sampler_rollout: obs is optional elsewhere)
    ("missing state_out", dict(state_out=None), EINVAL, BATCH),
    ("missing xfrag", dict(xfrag=None), EINVAL, BATCH),
    # two things wrong at once: the argument rules come before the config, the config before the
    # batch's pointers, lanes before everything
    ("policy 7 and a rack on the border", dict(policy=7, cfg=config(racks=(1, 8))), EINVAL, ANY),
    ("p > 1 and a null config", dict(p=1.5, cfg=None), EINVAL, ANY),
    ("rack on the border and no state", dict(cfg=config(racks=(1, 8)), state=None), ENOTSUP, ANY),
    ("bad lanes and a rack on the border", dict(lanes=3, cfg=config(racks=(1, 8))), EINVAL, ANY),
    ("bad order width and B < 0", dict(order_len=99, B=-1), EINVAL, ANY),
    # what is accepted: empty batches only
    ("empty batch", dict(), OK, ANY),
    ("order width 0 (= NA)", dict(order_len=0), OK, ANY),
    ("order width 1", dict(order_len=1), OK, ANY),
    ("order width 4 NA", dict(order_len=4 * NA), OK, ANY),
    ("every phase", dict(phase=nat.WH_PHASE_PRE_REGEN), OK, ANY),
    ("regeneration phase without actions", dict(phase=nat.WH_PHASE_REGEN, actions=None), OK, ANY),
    ("random policy, p = 1", dict(policy=nat.WH_POLICY_RANDOM, p=1.0), OK, ANY),
    ("lanes 1", dict(lanes=1), OK, ANY),
    ("lanes 16", dict(lanes=nat.WH_WIDE_LANES), OK, ANY),
]


def applies(name, over):
    if name != "wh_sampler_rollout" and "obs" in over:
        return False
    return all(k == "cfg" or k in ENTRIES[name] for k in over)


def forms(name, over, code, when):
    """(B, steps, expected code) of every form of a row for this entry point."""
    has_steps = "steps" in ENTRIES[name]
    some = over.get("steps", 3)
    out = []
    if code == OK:                       # accepted calls: the empty batch only
        out.append((0, some, OK))
        if has_steps:
            out.append((0, 0, OK))
    elif when == ANY:
        for B in ((over["B"],) if "B" in over else (0, 8)):
            out.append((B, some, code))
            if has_steps and "steps" not in over:
                out.append((B, 0, code))
    else:
        out.append((8, some, code))
        out.append((0, some, OK))
        if has_steps:
            out.append((0, 0, OK))
    return out


def call(lib, name, over, B, steps):
    """One call: every pointer a dummy (NULL for an empty batch), every option valid, then `over`."""
    vals = dict(cfg=config(), B=B, steps=steps, policy=nat.WH_POLICY_GREEDY, p=0.25, stats=None, autoreset=1,
                variable_n=0, seed=1234, env_offset=0, order_len=0, phase=nat.WH_PHASE_ALL, lanes=nat.WH_WIDE_LANES,
                stream=None, draws=None)
    for k in POINTERS:
        vals[k] = DUMMY if B > 0 else None
    handle = ctypes.c_void_p(0x1)
    vals["out"] = ctypes.byref(handle)
    vals.update({k: v for k, v in over.items() if k not in ("B", "steps")})
    for k in ("cfg", "stats", "draws"):
        if vals[k] is not None:
            vals[k] = ctypes.byref(vals[k])
    rc = getattr(lib, name)(*[vals[a] for a in ENTRIES[name]])
    if name == "wh_rollout_prepare" and vals["out"] is not None:
        if rc == OK and handle.value:
            assert lib.wh_launch_free(handle) == OK
        else:
            assert not handle.value, "a refused wh_rollout_prepare leaves *out NULL"
    return rc


def mismatches(lib, name, host):
    bad = []
    for what, over, code, when in TABLE:
        if not applies(name, over):
            continue
        for B, steps, want in forms(name, over, code, when):
            if host and name in HOST_ENOTSUP:
                want = ENOTSUP
            got = call(lib, name, over, B, steps)
            if got != want:
                bad.append(f"{name}({what}; B={B}, steps={steps}): returned {got}, contract {want}")
    return bad


@pytest.mark.parametrize("name", sorted(ENTRIES))
@pytest.mark.parametrize("engine", ["device", "host"])
def test_refusals(engine, name):
    host = engine == "host"
    bad = mismatches(nat.host_lib() if host else nat.lib(), name, host)
    assert not bad, "\n".join(bad)


# ---- rows of one entry point: (entry, what is wrong, the arguments, B, the device library's code, the
# host engine's).  The codes were read off both libraries before abi_args.h took these four entries
# over (pack_call / reset_call / observe_call), and are what they answered then.
def partial_draws(*given):
    return nat.WhResetDraws(*[DUMMY if k in given else None for k in ("spawn", "pickups", "targets", "n")])


OVERLAP = dict(racks=(4, 5))   # rack cells {3, 4} and {4, 5}: two pickup points on one cell
ENTRY_ROWS = []
for _name in ("wh_pack", "wh_unpack"):
    ENTRY_ROWS += [(_name, f"missing {k}", {k: None}, 8, EINVAL, EINVAL) for k in CANONICAL + ("state",)]
    ENTRY_ROWS += [
        # the empty batch is accepted before B < 0 and the pointers are looked at, the config is not
        (_name, "empty batch, no pointers", {}, 0, OK, OK),
        (_name, "B < 0 and a rack on the border", dict(cfg=config(racks=(1, 8))), -1, ENOTSUP, ENOTSUP),
        # the device's pack kernels need no tables, and an empty batch launches nothing
        (_name, "overlapping racks, empty batch", dict(cfg=config(**OVERLAP)), 0, OK, ENOTSUP),
        (_name, "overlapping racks", dict(cfg=config(**OVERLAP)), 8, None, ENOTSUP),
    ]
ENTRY_ROWS += [
    ("wh_reset", "draws without pickups", dict(draws=partial_draws("spawn", "targets")), 8, EINVAL, EINVAL),
    ("wh_reset", "draws without targets", dict(draws=partial_draws("spawn", "pickups", "n")), 8, EINVAL, EINVAL),
    ("wh_reset", "draws without spawn", dict(draws=partial_draws("pickups", "targets")), 8, EINVAL, EINVAL),
    ("wh_reset", "empty draws", dict(draws=partial_draws()), 8, EINVAL, EINVAL),
    ("wh_reset", "partial draws, empty batch", dict(draws=partial_draws("spawn")), 0, OK, OK),
    ("wh_reset", "partial draws and B < 0", dict(draws=partial_draws("spawn")), -1, EINVAL, EINVAL),
    ("wh_reset", "no mask (optional), empty batch", dict(mask=None), 0, OK, OK),
    ("wh_observe", "missing rows", dict(rows=None), 8, EINVAL, EINVAL),
    ("wh_observe", "missing rows, empty batch", dict(rows=None), 0, OK, OK),
    ("wh_observe_x", "neither rows nor xrows", dict(rows=None, xrows=None), 8, EINVAL, ENOTSUP),
    ("wh_observe_x", "misaligned xrows", dict(xrows=DUMMY + 4), 8, EINVAL, ENOTSUP),
    ("wh_observe_x", "misaligned xrows, no rows", dict(rows=None, xrows=DUMMY + 8), 8, EINVAL, ENOTSUP),
    ("wh_observe_x", "misaligned xrows and B < 0", dict(xrows=DUMMY + 4), -1, EINVAL, ENOTSUP),
    # (unlike wh_vector_step_x, whose xfrag is checked whatever the batch)
    ("wh_observe_x", "misaligned xrows, empty batch", dict(xrows=DUMMY + 4), 0, OK, ENOTSUP),
]
for _name in ("wh_reset", "wh_observe", "wh_observe_x"):
    ENTRY_ROWS += [
        # racks that overlap are a back end's refusal: the device library meets them when it builds the
        # tables of a batch that launches (not run here), the host engine in every call
        (_name, "overlapping racks, empty batch", dict(cfg=config(**OVERLAP)), 0, OK, ENOTSUP),
        (_name, "overlapping racks", dict(cfg=config(**OVERLAP)), 8, None, ENOTSUP),
    ]


@pytest.mark.parametrize("engine", ["device", "host"])
def test_entry_rows(engine):
    host = engine == "host"
    lib = nat.host_lib() if host else nat.lib()
    bad = []
    for name, what, over, B, dev_code, host_code in ENTRY_ROWS:
        want = host_code if host else dev_code
        if want is None:   # a call this library would launch
            continue
        got = call(lib, name, over, B, 1)
        if got != want:
            bad.append(f"{name}({what}; B={B}): returned {got}, contract {want}")
    assert not bad, "\n".join(bad)


def test_table_covers_every_entry():
    """Every row is used, and every entry point sees refusals, B > 0 refusals and an accepted call."""
    for what, over, code, when in TABLE:
        assert any(applies(n, over) for n in ENTRIES), what
    for name in ENTRIES:
        rows = [(code, B) for _, over, code, when in TABLE if applies(name, over)
                for B, _, code in forms(name, over, code, when)]
        assert sum(c != OK for c, _ in rows) >= 30 and any(c != OK and B > 0 for c, B in rows) and (OK, 0) in rows, name


def test_back_end_refusals_stay_apart():
    """A geometry the host engine runs and the device library has no kernel instance for is the one
    case where the two answer differently (an empty batch: nothing runs)."""
    cfg = nat.make_config(14, 9, (4, 8, 12), 8, 200, 200)
    for lib, want in ((nat.lib(), ENOTSUP), (nat.host_lib(), OK)):
        assert lib.wh_query(ctypes.byref(cfg), None) == want
        assert call(lib, "wh_step", dict(cfg=cfg), 0, 1) == want
        assert call(lib, "wh_rollout", dict(cfg=cfg), 0, 3) == want
        assert call(lib, "wh_sampler_rollout", dict(cfg=cfg), 0, 0) == want
