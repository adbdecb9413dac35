"""Test bodies of the sync-free learner's two entry points: wh_adam_step_clock (csrc/adam.h, the tick in
csrc/sac_formula.h) and wh_sac_td_la (csrc/sac.h); include/warehouse_amd.h, ADAM and SAC TD TARGETS.

tests/test_sync_free_cpu.py runs them on the host engine, tests/test_gpu_sync_free.py on the device.  The
buffers, the guards and the float64 model of wh_sac_td are tests/adam_cases.py's and tests/sac_cases.py's:
a proxy library hands their `lib.wh_sac_td(...)` call to wh_sac_td_la with a log_alpha pointer, so the two
entry points run on the very same buffers.

The clock's table against _native.adam_hyper (pow): beta^t as a running product of t correctly rounded
double multiplications differs from the correctly rounded power by at most about t * 2^-53 relative, which
for t <= 2,000 is 2^-42 -- far below half an f32 ulp (2^-25 relative) -- so after the one rounding to f32
a field can differ from adam_hyper's only when the exact value lies that close to a rounding boundary,
and then by one f32 ulp.  At t = 1 the product is beta * 1.0 = beta exactly: the tables are equal.

The TD bound with alpha read on the device: sac_cases.bounds(NA, alpha, discount) for alpha =
exp(log_alpha), widened by discount * ln 9 * 2 ulp(alpha) -- alpha multiplies sum_o p |log p| <= ln 9,
and expf is a 2-ulp function on either engine.
"""
import ctypes

import numpy as np
import torch

import adam_cases as ac
import sac_cases as sc

GUARD = 256
LRS = (1e-4, 3e-4)
T_MAX = 2000
HYPER = ("beta1", "omb1", "beta2", "omb2", "eps", "step_size", "sqrt_bc2")
LOG_ALPHAS = (float(np.log(0.2)), -3.0, 1.0)
TD_NAS = (1, 4, 8, 16)
TD_MS = (1, 33)          # one sample; a count that leaves a partial last workgroup at every NA (256 / NA > 1)


# ----------------------------------------------------------------------------- the clock
def table(h):
    """A wh_adam_hyper's seven f32 fields as an array."""
    return np.array([getattr(h, k) for k in HYPER], np.float32)


def ulps(a, b):
    """Distance in f32 steps between two arrays of positive f32 values."""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def model_tick(c, lr, betas, eps):
    """The header's tick on (t, beta1^t, beta2^t) in Python floats (IEEE double, one operation at a
    time): the new triple and the seven values each rounded to f32 once."""
    t, b1t, b2t = c[0] + 1, c[1] * betas[0], c[2] * betas[1]
    h = np.array([betas[0], 1.0 - betas[0], betas[1], 1.0 - betas[1], eps, lr / (1.0 - b1t), np.sqrt(1.0 - b2t)],
                 np.float64).astype(np.float32)
    return (t, b1t, b2t), h


class Clock:
    """A wh_adam_clock in a guarded buffer of one engine, 8-byte aligned (or `offset` bytes off)."""

    def __init__(self, nat, device, t=0, betas=ac.BETAS, offset=0):
        self.nat, self.size = nat, ctypes.sizeof(nat.WhAdamClock)
        self.raw = torch.full((GUARD + offset + self.size + GUARD,), 0xA5, dtype=torch.uint8, device=device)
        assert self.raw.data_ptr() % 16 == 0
        self.o = GUARD + offset
        self.raw[self.o:self.o + self.size] = torch.frombuffer(bytearray(bytes(nat.adam_clock(t, *betas))),
                                                               dtype=torch.uint8).to(device)

    @property
    def ptr(self):
        return self.raw.data_ptr() + self.o

    def read(self):
        h = self.raw.cpu().numpy()
        assert (h[:self.o] == 0xA5).all() and (h[self.o + self.size:] == 0xA5).all(), "bytes written outside the clock"
        return self.nat.WhAdamClock.from_buffer_copy(h[self.o:self.o + self.size].tobytes())


def fields(c):
    """(t, beta1_t, beta2_t as bits, the table as bits): what two engines' clocks are compared by (the
    struct's four bytes of tail padding are nobody's)."""
    return (int(c.t), np.float64(c.beta1_t).view(np.uint64), np.float64(c.beta2_t).view(np.uint64),
            tuple(table(c.h).view(np.uint32)))


def seg_array(run, nseg=None):
    nat = run.nat
    n = len(run.segments) if nseg is None else nseg
    arr = (nat.WhAdamSeg * max(1, n))()
    for i in range(n):
        b = run.buf[i]
        arr[i] = nat.WhAdamSeg(*[b[k][0].data_ptr() + b[k][1] for k in ("p", "m", "v", "g")], run.segments[i][0])
    return n, arr


def clock_step(run, clock, lr=ac.LR, betas=ac.BETAS, eps=ac.EPS, nseg=None):
    """wh_adam_step_clock of `run`'s library on its segments."""
    n, arr = seg_array(run, nseg)
    rc = run.lib.wh_adam_step_clock(n, arr, clock.ptr, lr, betas[0], betas[1], eps,
                                    run.nat.stream_of(torch.device(run.device)))
    assert rc == run.nat.WH_OK, rc


def hyper_step(run, h):
    """wh_adam_step of `run`'s library with the table `h`."""
    n, arr = seg_array(run)
    rc = run.lib.wh_adam_step(n, arr, ctypes.byref(h), run.nat.stream_of(torch.device(run.device)))
    assert rc == run.nat.WH_OK, rc


def same_tensors(a, b, what):
    for (count, off, goff), x, y in zip(ac.SEGMENTS, a, b):
        for key in ("p", "m", "v"):
            same = x[key].view(np.uint32) == y[key].view(np.uint32)
            assert same.all(), f"{what}, segment of {count} at offsets {off}/{goff}: {key} differs at {np.flatnonzero(~same)[:4]}"


def case_model_against_pow(nat, lr):
    """The model alone: equal to adam_hyper at t = 1, within one f32 ulp per field up to T_MAX.
    Returns the largest distance seen."""
    c, worst = (0, 1.0, 1.0), 0
    for t in range(1, T_MAX + 1):
        c, h = model_tick(c, lr, ac.BETAS, ac.EPS)
        d = ulps(h, table(nat.adam_hyper(lr, ac.BETAS[0], ac.BETAS[1], ac.EPS, t)))
        assert d.max() <= 1, f"model, lr {lr}, t {t}: {dict(zip(HYPER, d))}"
        assert t > 1 or d.max() == 0, f"model, lr {lr}: the table of t = 1 differs from adam_hyper's"
        worst = max(worst, int(d.max()))
    return worst


def case_clock_against_pow(nat, lib, device, lr):
    """T_MAX chained ticks (nseg = 0 still ticks) of one engine: t counts, the products and the table are
    the model's bit for bit, and the table is adam_hyper's at t = 1 and within one f32 ulp after."""
    clock = Clock(nat, device)
    c = (0, 1.0, 1.0)
    stream = nat.stream_of(torch.device(device))
    for t in range(1, T_MAX + 1):
        assert lib.wh_adam_step_clock(0, None, clock.ptr, lr, ac.BETAS[0], ac.BETAS[1], ac.EPS, stream) == nat.WH_OK
        got = clock.read()
        c, h = model_tick(c, lr, ac.BETAS, ac.EPS)
        assert (got.t, got.beta1_t, got.beta2_t) == c, f"lr {lr}, t {t}: the clock is not the model's"
        assert np.array_equal(table(got.h).view(np.uint32), h.view(np.uint32)), f"lr {lr}, t {t}: the table is not the model's"
        d = ulps(table(got.h), table(nat.adam_hyper(lr, ac.BETAS[0], ac.BETAS[1], ac.EPS, t)))
        assert d.max() <= 1 and (t > 1 or d.max() == 0), f"lr {lr}, t {t}: {dict(zip(HYPER, d))}"


def case_step_is_adam_step_with_the_clocks_table(nat, lib, device, t0, seed=0):
    """One wh_adam_step_clock from a clock at t0 on adam_cases' 24 segments (the unaligned and the empty
    ones included) leaves the tensors wh_adam_step leaves when called with clock.h, bit for bit."""
    state = ac.make_state(seed + t0)
    a, b = ac.Run(nat, lib, device, state), ac.Run(nat, lib, device, state)
    clock = Clock(nat, device, t=t0)
    clock_step(a, clock)
    got = clock.read()
    assert got.t == t0 + 1
    hyper_step(b, got.h)
    same_tensors(a.get(), b.get(), f"one call from t = {t0}")
    return got


def case_engines_agree_on_the_clock(nat, steps=20, t0=0, seed=0):
    """`steps` chained wh_adam_step_clock calls with fresh gradients each, on the device and on the host
    engine: the clock (t, both products, the table) and p, m, v equal bit for bit after the first call and
    after the last."""
    state = ac.make_state(seed + t0)
    dev, host = ac.Run(nat, nat.lib(), "cuda:0", state), ac.Run(nat, nat.host_lib(), "cpu", state)
    cd, ch = Clock(nat, "cuda:0", t=t0), Clock(nat, "cpu", t=t0)
    for k in range(steps):
        if k:
            g = [dict(g=x) for x in ac.fresh_gradients(seed + 100 * t0 + k)]
            dev.put(g, ("g",))
            host.put(g, ("g",))
        clock_step(dev, cd)
        clock_step(host, ch)
        if k in (0, steps - 1):
            x, y = cd.read(), ch.read()
            assert x.t == t0 + k + 1 and fields(x) == fields(y), f"call {k + 1}: clocks differ: {fields(x)} / {fields(y)}"
            same_tensors(dev.get(), host.get(), f"call {k + 1} from t = {t0}")


def case_clock_refusals(nat, lib, host: bool):
    """The refusals of wh_adam_step_clock as (what, code) of one library.  Refused calls never touch a
    pointer, so the device library gets dummies; the calls that are WH_OK tick, so they are made on the
    host engine alone (real memory) and checked there."""
    E, OK = nat.WH_EINVAL, nat.WH_OK
    clock = Clock(nat, "cpu") if host else None
    cp = clock.ptr if host else 0x10000
    good = [0x20000, 0x30000, 0x40000, 0x50000]

    def call(nseg=2, clk=cp, null_segs=False, second=None):
        arr = (nat.WhAdamSeg * 25)()
        for i in range(25):
            arr[i] = nat.WhAdamSeg(*good, 0)
        if second is not None:
            arr[1] = nat.WhAdamSeg(*second)
        return lib.wh_adam_step_clock(nseg, None if null_segs else arr, clk, ac.LR, ac.BETAS[0], ac.BETAS[1], ac.EPS, None)

    table_ = [("nseg -1", call(nseg=-1), E), ("nseg 25", call(nseg=25), E), ("NULL clock", call(clk=None), E),
              ("NULL clock, nseg 0", call(nseg=0, clk=None), E), ("NULL segs", call(null_segs=True), E),
              ("count -1", call(second=good + [-1]), E)]
    for o in (1, 2, 4):
        table_.append((f"clock at offset {o}", call(clk=cp + o), E))
    for i, k in enumerate(("p", "m", "v", "g")):
        s = good + [6]
        s[i] = None
        table_.append((f"NULL {k}", call(second=s), E))
        for o in (1, 2, 3):
            s = good + [6]
            s[i] = good[i] + o
            table_.append((f"{k} at offset {o}", call(second=s), E))
    for what, rc, want in table_:
        assert rc == want, f"{what}: got {rc}, expected {want}"
    if host:
        assert clock.read().t == 0, "a refused call ticked"
        for n, (what, kw) in enumerate((("nseg 0", dict(nseg=0)), ("nseg 0, NULL segs", dict(nseg=0, null_segs=True)),
                                        ("24 empty segments", dict(nseg=24)),
                                        ("count 0 with NULL pointers", dict(second=[None, None, None, None, 0])))):
            rc = call(**kw)
            assert rc == OK, f"{what}: got {rc}"
            assert clock.read().t == n + 1, f"{what}: a call without elements still ticks"
    return [(what, rc) for what, rc, _ in table_]


# ----------------------------------------------------------------------------- TD targets with alpha read in place
class LaLib:
    """`lib` with wh_sac_td answered by wh_sac_td_la reading `log_alpha` (a one-element f32 tensor of the
    engine's memory, or a raw address): sac_cases' bodies then drive the new entry point on their own
    buffers."""

    def __init__(self, lib, log_alpha):
        self.lib, self.log_alpha = lib, log_alpha

    def wh_sac_td(self, M, NA, args, stream):
        la = self.log_alpha
        return self.lib.wh_sac_td_la(M, NA, args, la.data_ptr() if torch.is_tensor(la) else la, stream)


def options(inp0, M, NA):
    """sac_cases.OPTIONS as (name, inputs, mask, offset, outputs, L), without their alpha."""
    for name, twin_t, nq, use_n, mask, _, offset, *rest in sc.OPTIONS:
        L = rest[0] if rest else sc.L_LOGIT
        inp = dict(inp0)
        if L == sc.L_PEAKED:
            inp["pi_next"] = sc.peaked_logits(M * NA, 1000 * NA + M)
        if not twin_t:
            inp["q2t_next"] = None
        if nq < 2:
            inp["q2"] = None
        if nq < 1:
            inp["q1"] = None
        if not use_n:
            inp["n"] = None
        if not mask:
            inp = dict(inp, dones=inp["dones"] if offset else None)
        yield name, inp, mask, offset, (("y", "td_rows", "td") if nq else ("y",)), L


def case_td_la(nat, lib, device, NA, M):
    """Every option case of sac_cases at one (NA, M): at log_alpha = 0 wh_sac_td_la's outputs are
    wh_sac_td's at alpha = 1 bit for bit (args.alpha, which it must ignore, is NaN); at the LOG_ALPHAS they
    stay within the widened bounds of the float64 model at alpha = exp(log_alpha).  Returns the largest
    errors seen as fractions of the bounds."""
    inp0 = sc.make_inputs(M, NA, 1000 * NA + M)
    worst = {}
    for name, inp, mask, offset, outputs, L in options(inp0, M, NA):
        kw = dict(discount=sc.DISCOUNT, mask_dones=mask, offset=offset, outputs=outputs)
        zero = torch.zeros(1, dtype=torch.float32, device=device)
        got = sc.run_td(nat, LaLib(lib, zero), device, M, NA, inp, alpha=float("nan"), **kw)
        ref = sc.run_td(nat, lib, device, M, NA, inp, alpha=1.0, **kw)
        for k in outputs:
            assert np.array_equal(got[k].view(np.uint32), ref[k].view(np.uint32)), \
                f"NA={NA} M={M} [{name}] {k}: log_alpha = 0 is not alpha = 1"
        for la in LOG_ALPHAS:
            t = torch.full((1,), la, dtype=torch.float32, device=device)
            got = sc.run_td(nat, LaLib(lib, t), device, M, NA, inp, alpha=float("nan"), **kw)
            alpha = np.float32(np.exp(np.float64(np.float32(la))))
            want = dict(zip(("y", "td_rows", "td"), sc.model(inp, NA, alpha=alpha, discount=sc.DISCOUNT, mask_dones=mask)))
            by, btd = sc.bounds(NA, float(alpha), np.float32(sc.DISCOUNT), L=L)
            wide = float(np.float32(sc.DISCOUNT)) * np.log(9.0) * 2 * float(np.spacing(alpha))
            for k in outputs:
                err = float(np.abs(got[k].astype(np.float64) - want[k]).max())
                b = (btd if k == "td" else by) + wide
                worst[k] = max(worst.get(k, 0.0), err / b)
                assert err <= b, f"NA={NA} M={M} [{name}] log_alpha {la} {k}: error {err:.3e}, bound {b:.3e}"
    return worst


def case_td_la_refusals(nat, lib, host: bool):
    """wh_sac_td's refusal table through wh_sac_td_la with a valid log_alpha (sac_cases.case_refusals
    asserts the codes; refused and M = 0 calls touch nothing and launch nothing), then log_alpha == NULL."""
    la = torch.full((1,), 0.5, dtype=torch.float32)
    codes = sc.case_refusals(nat, LaLib(lib, la if host else 0x7000), host)   # (a dummy address for the device library)
    assert float(la[0]) == 0.5
    M, NA, rows = 3, 4, 12
    keep = [torch.full((36 * rows + 64,), 0xA5, dtype=torch.uint8) for _ in range(6)] if host else None
    p = [t.data_ptr() for t in keep] if host else [4096 * (i + 1) for i in range(6)]
    args = nat.WhSacTdArgs(pi_next=p[0], q1t_next=p[1], actions=p[2], rewards=p[3], alpha=0.2, discount=0.99, y=p[4])
    extra = [("NULL log_alpha", lib.wh_sac_td_la(M, NA, ctypes.byref(args), None, None), nat.WH_EINVAL),
             ("NULL log_alpha, M = 0", lib.wh_sac_td_la(0, NA, ctypes.byref(args), None, None), nat.WH_OK),
             ("NULL log_alpha and NULL args", lib.wh_sac_td_la(M, NA, None, None, None), nat.WH_EINVAL)]
    for what, rc, want in extra:
        assert rc == want, f"{what}: got {rc}, expected {want}"
    assert keep is None or all(bool((t == 0xA5).all()) for t in keep), "a refused (or empty) call wrote to a buffer"
    return codes + [(what, rc) for what, rc, _ in extra]
