"""Test bodies of wh_sac_loss (csrc/sac_loss.h, csrc/sac_formula.h; include/warehouse_amd.h, SAC LOSSES).

tests/test_gpu_loss.py runs them on the GPU, tests/test_loss_cpu.py on the host engine.  The bodies take
`(lib, device)` and go through the C ABI with 0xA5 guards before and behind every output, as
sac_cases.run_td does.  The model is numpy float64 of the header's formula, written here.

Bounds (derived, nothing measured went into them).  Inputs: |pi| <= L, |q| <= Qm, |y| <= Ym, 0 < w <= 1,
alpha = exp(log_alpha).  With G = alpha (2 L + ln 9) + Qm (the largest |g[o]| and |f|), E = 2 L + ln 9 +
|target_entropy| (the largest |logp + te|), C = 0.5 (Qm + Ym)^2 (the largest c_k) and R = M NA rows:
  dpi          64 * 2^-24 * 2 G * scale      p <= 1, |g - f| <= 2 G; the lse, the exps and the 9-term sum
                                             cost a few units of 2^-24 relative to G each; 64 leaves room
                                             for 2-ulp device expf / logf
  dq           8 * 2^-24 * (Qm + Ym) * scale one subtraction and two products
  the sums     (64 + 256 + workgroups) * 2^-24 * scale * R * {C, G, E}: every term carries the row's 64,
                                             and a sum at most 256 + workgroups additions deep adds one
                                             unit of 2^-24 of the running total per addition
  alpha_loss   the bound of T times |log_alpha|, plus one ulp of the result
"""
import ctypes

import numpy as np
import torch

import sac_cases as sc
from sac_cases import _guarded, _place

L_LOGIT, QM, YM = 4.0, 10.0, 20.0
LOG_ALPHA = float(np.log(0.2))
TARGET_ENTROPY = 0.935
EPS24 = 2.0 ** -24
STAT_KEYS = ("critic1", "critic2", "actor", "alpha_loss", "dalpha", "live")


def groups_of(M, NA):
    spw = 256 // NA
    return (M + spw - 1) // spw


# ----------------------------------------------------------------------------- the model
def model(inp, NA, *, log_alpha, target_entropy, scale, dtype=np.float64):
    """(dpi, dq1, dq2 [rows, 9], stats [6]) of the header's formula in `dtype`, the sums in ascending row
    order; dq2 is None without q2.  log_alpha, target_entropy and scale enter as the f32 values the ABI
    takes."""
    f = dtype
    la, te, sc_ = f(np.float32(log_alpha)), f(np.float32(target_entropy)), f(np.float32(scale))
    alpha = np.exp(la).astype(f)
    pi, q1 = inp["pi"].astype(f), inp["q1"].astype(f)
    q2 = None if inp.get("q2") is None else inp["q2"].astype(f)
    rows = pi.shape[0]
    M = rows // NA
    n = np.full(M, NA) if inp.get("n") is None else np.clip(inp["n"].astype(np.int64), 0, NA)
    live = (np.arange(NA)[None, :] < n[:, None]).reshape(rows)
    w = np.ones(M, f) if inp.get("weights") is None else inp["weights"].astype(f)
    w = np.repeat(w, NA)
    y = inp["y"].astype(f).reshape(rows)
    a = inp["actions"].astype(np.int64).reshape(rows)
    a = np.where((a >= 0) & (a < 9), a, 4)
    zmax = pi.max(axis=1)
    s = np.zeros(rows, f)
    for o in range(9):
        s = s + np.exp(pi[:, o] - zmax)
    lse = zmax + np.log(s)
    logp = (pi - lse[:, None]).astype(f)
    p = np.exp(logp).astype(f)
    qm = q1 if q2 is None else np.minimum(q1, q2)
    g = (alpha * logp - qm).astype(f)
    fa, t = np.zeros(rows, f), np.zeros(rows, f)
    for o in range(9):
        fa = fa + p[:, o] * g[:, o]
        t = t + p[:, o] * (logp[:, o] + te)
    dpi = ((sc_ * p) * (g - fa[:, None])).astype(f)
    r = np.arange(rows)
    onehot = np.zeros((rows, 9), bool)
    onehot[r, a] = True

    def critic(q):
        e = q[r, a] - y
        c = ((f(0.5) * w) * e) * e
        return c, np.where(onehot, ((sc_ * w) * e)[:, None], f(0)).astype(f)

    c1, dq1 = critic(q1)
    c2, dq2 = critic(q2) if q2 is not None else (np.zeros(rows, f), None)
    dead = ~live
    dpi[dead], dq1[dead] = 0, 0
    if dq2 is not None:
        dq2[dead] = 0

    def total(x):   # ascending row order, in `dtype`
        x = np.where(live, x, f(0)).astype(f)
        return np.cumsum(x, dtype=f)[-1] if rows else f(0)

    T = sc_ * total(t)
    stats = np.array([sc_ * total(c1), sc_ * total(c2), sc_ * total(fa), (-la) * T, -T, f(live.sum())], f)
    return dpi, dq1, dq2, stats


def bounds(M, NA, *, alpha, log_alpha, target_entropy, scale, L=L_LOGIT, Qm=QM, Ym=YM):
    """dict: dpi, dq, and the bounds of stats[0..4] (alpha_loss without its one ulp)."""
    G = alpha * (2 * L + np.log(9.0)) + Qm
    E = 2 * L + np.log(9.0) + abs(target_entropy)
    C = 0.5 * (Qm + Ym) ** 2
    depth = (64 + 256 + groups_of(M, NA)) * EPS24 * scale * (M * NA)
    return dict(dpi=64 * EPS24 * 2 * G * scale, dq=8 * EPS24 * (Qm + Ym) * scale, critic1=depth * C, critic2=depth * C,
                actor=depth * G, dalpha=depth * E, alpha_loss=depth * E * abs(log_alpha))


def make_inputs(M, NA, seed):
    """sac_cases.make_inputs' logits, Q values, actions (strays -3 and 9 planted) and n (mixing -1, 0,
    partial counts and NA); y uniform in [-20, 20], weights in [0.25, 1]."""
    base = sc.make_inputs(M, NA, seed)
    rng = np.random.default_rng(seed + 77)
    return dict(pi=base["pi_next"], q1=base["q1"], q2=base["q2"], actions=base["actions"], n=base["n"],
                y=rng.uniform(-YM, YM, (M, NA)).astype(np.float32),
                weights=rng.uniform(0.25, 1.0, M).astype(np.float32))


# option cases: (name, twin, use n, use weights, byte offset of every input, byte offset of every output, outputs
# [, the bound L of |pi|: sac_cases.L_PEAKED takes peaked_logits])
ALL = ("dpi", "dq1", "dq2")
OPTIONS = (
    ("twin, n, weights", True, True, True, 0, 0, ALL),
    ("single Q, n = NULL, weights = NULL, every array at offset 4", False, False, False, 4, 4, ("dpi", "dq1")),
    ("twin, n, weights, outputs at offset 4 of inputs at 0", True, True, True, 0, 4, ALL),
    ("twin, n, weights = NULL, outputs at offset 0 of inputs at 4", True, True, False, 4, 0, ALL),
    ("peaked policies, twin, n, weights, offset 4", True, True, True, 4, 4, ALL, sc.L_PEAKED),
    ("twin, n, weights, dq1 alone", True, True, True, 0, 4, ("dq1",)),
    ("twin, n = NULL, weights, dpi and dq2, offset 4", True, False, True, 4, 4, ("dpi", "dq2")),
    ("single Q, n, weights, no gradient output", False, True, True, 0, 0, ()),
)


def run_loss(nat, lib, device, M, NA, inp, *, log_alpha, target_entropy, scale, in_off=0, out_off=0, outputs=ALL):
    """wh_sac_loss of one library on `inp` (None entries = NULL); the outputs as numpy, their guard
    bytes (before and behind) checked, `work`'s too."""
    keep, ptr = {}, {}
    arrays = dict(inp, log_alpha=np.array([log_alpha], np.float32))
    for k in ("pi", "q1", "q2", "y", "actions", "n", "weights", "log_alpha"):
        if arrays.get(k) is None:
            ptr[k] = None
        else:
            keep[k] = _place(arrays[k], device, in_off)
            ptr[k] = keep[k].data_ptr() + in_off
    rows = M * NA
    sizes = dict(dpi=36 * rows, dq1=36 * rows, dq2=36 * rows, stats=24)
    out = {k: _guarded(sizes[k], device, out_off) for k in tuple(outputs) + ("stats",)}
    nbytes = ctypes.c_int64()
    assert lib.wh_sac_loss_query(M, NA, ctypes.byref(nbytes)) == nat.WH_OK and nbytes.value > 0
    work = _guarded(int(nbytes.value), device, 0)
    args = nat.WhSacLossArgs(ptr["pi"], ptr["q1"], ptr["q2"], ptr["y"], ptr["actions"], ptr["n"], ptr["weights"],
                             ptr["log_alpha"], target_entropy, scale,
                             *[(out[k].data_ptr() + out_off) if k in out else None for k in ALL + ("stats",)],
                             work.data_ptr())
    rc = lib.wh_sac_loss(M, NA, ctypes.byref(args), nat.stream_of(torch.device(device)))
    assert rc == nat.WH_OK, rc
    res = {}
    for k, t in out.items():
        h = t.cpu().numpy()
        assert (h[:out_off] == 0xA5).all() and (h[out_off + sizes[k]:] == 0xA5).all(), f"bytes written outside {k}"
        res[k] = h[out_off:out_off + sizes[k]].copy().view(np.float32).reshape((rows, 9) if k != "stats" else (6,))
    assert (work.cpu().numpy()[int(nbytes.value):] == 0xA5).all(), "bytes written behind work"
    return res


def case_loss(nat, lib, device, NA, M, quarter=False):
    """Every option case at one (NA, M) against the float64 model, within the stated bounds (a quarter
    of them with `quarter`: what the host engine must keep); exact zeros on dead rows; stats[5] exact.
    Returns the largest errors seen, as fractions of the bounds."""
    inp0 = make_inputs(M, NA, 1000 * NA + M)
    scale = 1.0 / (M * NA)
    worst = {}
    frac = 0.25 if quarter else 1.0
    for name, twin, use_n, use_w, in_off, out_off, outputs, *rest in OPTIONS:
        L = rest[0] if rest else L_LOGIT
        inp = dict(inp0)
        if L == sc.L_PEAKED:
            inp["pi"] = sc.peaked_logits(M * NA, 1000 * NA + M)
        assert float(np.abs(inp["pi"]).max()) <= L
        if not twin:
            inp["q2"] = None
        if not use_n:
            inp["n"] = None
        if not use_w:
            inp["weights"] = None
        got = run_loss(nat, lib, device, M, NA, inp, log_alpha=LOG_ALPHA, target_entropy=TARGET_ENTROPY, scale=scale,
                       in_off=in_off, out_off=out_off, outputs=outputs)
        dpi, dq1, dq2, stats = model(inp, NA, log_alpha=LOG_ALPHA, target_entropy=TARGET_ENTROPY, scale=scale)
        want = dict(dpi=dpi, dq1=dq1, dq2=dq2)
        b = bounds(M, NA, alpha=0.2, log_alpha=LOG_ALPHA, target_entropy=TARGET_ENTROPY, scale=np.float32(scale), L=L)
        pre = "" if L == L_LOGIT else "peaked "
        for k in outputs:
            err = float(np.abs(got[k].astype(np.float64) - want[k]).max())
            bk = b["dpi"] if k == "dpi" else b["dq"]
            worst[pre + k] = max(worst.get(pre + k, 0.0), err / bk)
            assert err <= frac * bk, f"NA={NA} M={M} [{name}] {k}: error {err:.3e}, bound {frac * bk:.3e}"
        for j, k in enumerate(STAT_KEYS[:5]):
            err = abs(float(got["stats"][j]) - float(stats[j]))
            ulp = float(np.spacing(np.float32(abs(stats[j])))) if k == "alpha_loss" else 0.0
            worst[pre + k] = max(worst.get(pre + k, 0.0), err / b[k])
            assert err <= frac * b[k] + ulp, f"NA={NA} M={M} [{name}] {k}: error {err:.3e}, bound {frac * b[k]:.3e}"
        n = np.full(M, NA) if inp["n"] is None else inp["n"]
        live = np.arange(NA)[None, :] < np.clip(n, 0, NA)[:, None]
        assert float(got["stats"][5]) == float(live.sum()), f"[{name}] stats[5]"
        if not twin:
            assert got["stats"][1] == 0.0
        dead = ~live.reshape(-1)
        for k in outputs:
            assert (got[k][dead] == 0.0).all(), f"[{name}] {k} of dead rows"
    return worst


def case_float32_model(NA, M):
    """The float32 numpy transcription of the formula stays under a quarter of the bounds on the test's
    own inputs (if it did not, the operation order would be wrong, not the bound)."""
    inp0 = make_inputs(M, NA, 1000 * NA + M)
    scale = 1.0 / (M * NA)
    worst = {}
    for L in (L_LOGIT, sc.L_PEAKED):
        inp = inp0 if L == L_LOGIT else dict(inp0, pi=sc.peaked_logits(M * NA, 1000 * NA + M))
        kw = dict(log_alpha=LOG_ALPHA, target_entropy=TARGET_ENTROPY, scale=scale)
        a, b64 = model(inp, NA, dtype=np.float32, **kw), model(inp, NA, **kw)
        b = bounds(M, NA, alpha=0.2, log_alpha=LOG_ALPHA, target_entropy=TARGET_ENTROPY, scale=np.float32(scale), L=L)
        pre = "" if L == L_LOGIT else "peaked "
        for k, x, w in zip(("dpi", "dq1", "dq2"), a[:3], b64[:3]):
            err = float(np.abs(x.astype(np.float64) - w).max())
            bk = b["dpi"] if k == "dpi" else b["dq"]
            worst[pre + k] = max(worst.get(pre + k, 0.0), err / bk)
            assert err <= 0.25 * bk, f"float32 model NA={NA} M={M} L={L} {k}: {err:.3e} > {0.25 * bk:.3e}"
        for j, k in enumerate(STAT_KEYS[:5]):
            err = abs(float(a[3][j]) - float(b64[3][j]))
            ulp = float(np.spacing(np.float32(abs(b64[3][j])))) if k == "alpha_loss" else 0.0
            worst[pre + k] = max(worst.get(pre + k, 0.0), err / b[k])
            assert err <= 0.25 * b[k] + ulp, f"float32 model NA={NA} M={M} L={L} {k}: {err:.3e} > {0.25 * b[k]:.3e}"
        assert a[3][5] == b64[3][5]
    return worst


# ----------------------------------------------------------------------------- exact sums
def case_exact(nat, lib, device, NA, M):
    """Answers that are exact in any summation order: every pi row one logit at +200 and eight at 0 (p
    exactly one-hot, logp 0 at the peak), q and y integers in [-8, 8], w in {0.25, 0.5, 1}, scale 2^-10,
    target_entropy 0.5, log_alpha -1.  A live row adds -qm[r, peak] to the actor sum, 0.5 to the alpha sum
    and a multiple of 1/8 to each critic sum; all partial sums stay below 2^24 in units of 2^-13.  stats
    equal the integer model bit for bit, dq equals scale w e exactly, every dpi element compares equal to 0."""
    rng = np.random.default_rng(31 * NA + M)
    rows = M * NA
    peak = rng.integers(0, 9, rows)
    pi = np.zeros((rows, 9), np.float32)
    pi[np.arange(rows), peak] = 200.0
    base = sc.make_inputs(M, NA, 1000 * NA + M)
    inp = dict(pi=pi, q1=rng.integers(-8, 9, (rows, 9)).astype(np.float32),
               q2=rng.integers(-8, 9, (rows, 9)).astype(np.float32), y=rng.integers(-8, 9, (M, NA)).astype(np.float32),
               actions=base["actions"], n=base["n"], weights=rng.choice(np.array([0.25, 0.5, 1.0], np.float32), M))
    scale, te, la = 2.0 ** -10, 0.5, -1.0
    live = (np.arange(NA)[None, :] < np.clip(inp["n"], 0, NA)[:, None]).reshape(rows)
    a = inp["actions"].reshape(rows).astype(np.int64)
    a = np.where((a >= 0) & (a < 9), a, 4)
    r = np.arange(rows)
    w = np.repeat(inp["weights"].astype(np.float64), NA)
    for twin in (True, False):
        cur = dict(inp) if twin else dict(inp, q2=None)
        got = run_loss(nat, lib, device, M, NA, cur, log_alpha=la, target_entropy=te, scale=scale, in_off=4, out_off=0,
                       outputs=ALL if twin else ("dpi", "dq1"))
        q1, q2 = inp["q1"].astype(np.float64), inp["q2"].astype(np.float64)
        qm = np.minimum(q1, q2) if twin else q1
        y = inp["y"].astype(np.float64).reshape(rows)
        e1, e2 = q1[r, a] - y, q2[r, a] - y
        T = scale * 0.5 * live.sum()
        want = np.array([scale * (0.5 * w * e1 * e1)[live].sum(), scale * (0.5 * w * e2 * e2)[live].sum() if twin else 0.0,
                         scale * (-qm[r, peak])[live].sum(), T, -T, live.sum()], np.float64)
        assert np.abs(want[:5]).max() * 2 ** 13 < 2 ** 24 and (want * 2 ** 13 == np.round(want * 2 ** 13)).all()
        assert np.array_equal(got["stats"].astype(np.float64), want), f"NA={NA} M={M} twin={twin}: {got['stats']} != {want}"
        assert (got["dpi"] == 0.0).all()
        for k, e in (("dq1", e1), ("dq2", e2)):
            if k not in got:
                continue
            d = np.zeros((rows, 9))
            d[r, a] = np.where(live, scale * w * e, 0.0)
            assert np.array_equal(got[k].astype(np.float64), d), f"NA={NA} M={M} twin={twin}: {k}"


def case_deterministic(nat, lib, device, NA, M):
    """Two calls on the same inputs give equal bytes."""
    inp = make_inputs(M, NA, 5 * NA + M)
    kw = dict(log_alpha=LOG_ALPHA, target_entropy=TARGET_ENTROPY, scale=1.0 / (M * NA), in_off=0, out_off=4)
    a, b = run_loss(nat, lib, device, M, NA, inp, **kw), run_loss(nat, lib, device, M, NA, inp, **kw)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


# ----------------------------------------------------------------------------- refusals
def case_refusals(nat, lib, host: bool):
    """The refusals of wh_sac_loss and wh_sac_loss_query (codes of one library as a list, compared between
    the libraries by the caller).  On the host engine every pointer is a real sentinel-filled buffer that
    must stay untouched; on the device library dummies a refused or empty call never dereferences."""
    M, NA = 3, 4
    keep = []

    def mem(nbytes):
        if not host:
            keep.append(None)
            return 4096 * len(keep)
        t = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8)
        assert t.data_ptr() % 16 == 0
        keep.append(t)
        return t.data_ptr()

    rows = M * NA
    base = dict(pi=mem(36 * rows), q1=mem(36 * rows), q2=mem(36 * rows), y=mem(4 * rows), actions=mem(4 * rows),
                n=mem(4 * M), weights=mem(4 * M), log_alpha=mem(4), target_entropy=0.935, scale=1.0 / rows,
                dpi=mem(36 * rows), dq1=mem(36 * rows), dq2=mem(36 * rows), stats=mem(24), work=mem(64))

    def call(M_=M, NA_=NA, null_args=False, **over):
        a = dict(base, **over)
        return lib.wh_sac_loss(M_, NA_, None if null_args else ctypes.byref(nat.WhSacLossArgs(**a)), None)

    nb = ctypes.c_int64(-1)
    E, OK = nat.WH_EINVAL, nat.WH_OK
    pointers = [k for k in base if k not in ("target_entropy", "scale")]
    table = [
        ("NULL args", call(null_args=True), E),
        ("NULL args, M = 0", call(M_=0, null_args=True), E),
        ("M -1", call(M_=-1), E),
        ("NA 0", call(NA_=0), E),
        ("NA -2", call(NA_=-2), E),
        ("NA 17", call(NA_=17), E),
        ("NA 17, M = 0", call(M_=0, NA_=17), E),
        ("NULL pi", call(pi=None), E),
        ("NULL q1", call(q1=None), E),
        ("NULL y", call(y=None), E),
        ("NULL actions", call(actions=None), E),
        ("NULL log_alpha", call(log_alpha=None), E),
        ("NULL stats", call(stats=None), E),
        ("dq2 without q2", call(q2=None), E),
        ("NULL work", call(work=None), E),
        ("work at offset 4", call(work=base["work"] + 4), E),
        ("work at offset 8", call(work=base["work"] + 8), E),
        ("M = 0", call(M_=0), OK),
        ("M = 0, NULL arrays", call(M_=0, **{k: None for k in pointers}), OK),
        ("query M -1", lib.wh_sac_loss_query(-1, 4, ctypes.byref(nb)), E),
        ("query NA 0", lib.wh_sac_loss_query(3, 0, ctypes.byref(nb)), E),
        ("query NA 17", lib.wh_sac_loss_query(3, 17, ctypes.byref(nb)), E),
        ("query NULL out", lib.wh_sac_loss_query(3, 4, None), OK),
    ]
    assert nb.value == -1, "a refused query wrote work_bytes"
    for M_, NA_ in ((0, 4), (1, 16), (300, 9), (65, 8)):
        assert lib.wh_sac_loss_query(M_, NA_, ctypes.byref(nb)) == OK
        assert nb.value == 32 * max(1, groups_of(M_, NA_)) and nb.value % 16 == 0
        table.append((f"query {M_} {NA_}", int(nb.value), int(nb.value)))
    for what, rc, want in table:
        assert rc == want, f"{what}: got {rc}, expected {want}"
    for t in keep:
        assert t is None or bool((t == 0xA5).all()), "a refused (or empty) call wrote to a buffer"
    return [(what, rc) for what, rc, _ in table]
