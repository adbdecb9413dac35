"""Test bodies of the SAC forward half: wh_sac_td (csrc/sac.h, csrc/sac_formula.h) and
wh_mlp_pack_device (csrc/mlp_pack.h).

tests/test_gpu_sac.py runs them on the GPU, tests/test_sac_cpu.py runs the wh_sac_td bodies on the
host engine.  The wh_sac_td bodies take `(lib, device)` and go through the C ABI with sentinel guards
behind every output; the pack bodies need the device.  The model of wh_sac_td is numpy float64 of the
header's formula, written here.

Tolerances (from the issue, nothing measured went into them).  With S = max|r| + discount (Qm +
alpha (2 L + ln 9)) -- the largest |y| inputs bounded by L (logits), Qm (Q values) and max|r| allow:
  y, td_rows   64 * 2^-24 * S             each of the two 9-term sums, the log, the exps and the
                                          products costs a few units of 2^-24 relative to S; 64
                                          leaves room for 2-ulp device expf / logf
  td           2 (64 + NA) * 2^-24 * (S + Qm)   an NA-term mean of rows bounded by Qm + S
"""
import ctypes

import numpy as np
import torch

GUARD = 256
L_LOGIT, QM = 4.0, 10.0
REWARDS = np.array([-1.0, 0.0, 1.0, 10.0], np.float32)
L_PEAKED = 60.0
# A workgroup of k_sac_td owns floor(256 / NA) samples and stages its span of every [rows, 9] array
# with an unaligned head of 0-3 floats that depends on its first row.  NA = 1, 4, 9 and 16 make a
# span of 256, 256, 252 and 256 rows, a multiple of 16 bytes, so every block has the same head; NA =
# 3, 5, 10 and 11 make spans of 255, 255, 250 and 253 rows, whose float counts are 3, 3, 2 and 1
# mod 4, so the head changes from block to block through 1, 2 and 3.  NA = 2 and 8 (the headline's
# agent count) take the 16 % NA == 0 shuffle sum.  (tests/test_sac_cpu.py checks this arithmetic.)
NAS = (1, 2, 3, 4, 5, 8, 9, 10, 11, 16)
MS = (1, 65, 300)
BLOCK_ROWS = 256
DISCOUNT = 0.99 ** 3
EPS24 = 2.0 ** -24


# ----------------------------------------------------------------------------- the model
def model(inp, NA, *, alpha, discount, mask_dones, dtype=np.float64):
    """(y [M,NA], td_rows [M,NA], td [M]) of the header's formula in `dtype`; td_rows / td are None
    without q1.  inp: pi_next, q1t_next, q2t_next (or None), q1, q2 (or None) [M*NA, 9]; actions,
    rewards [M, NA]; dones, n [M] (or None).  alpha and discount enter as the f32 values the ABI takes."""
    f = dtype
    alpha, discount = f(np.float32(alpha)), f(np.float32(discount))
    pi, q1t = inp["pi_next"].astype(f), inp["q1t_next"].astype(f)
    q2t = None if inp.get("q2t_next") is None else inp["q2t_next"].astype(f)
    rows = pi.shape[0]
    M = rows // NA
    zmax = pi.max(axis=1)
    s = np.zeros(rows, f)
    for o in range(9):
        s = s + np.exp(pi[:, o] - zmax)
    lse = zmax + np.log(s)
    v = np.zeros(rows, f)
    for o in range(9):
        logp = pi[:, o] - lse
        p = np.exp(logp)
        q = q1t[:, o] if q2t is None else np.minimum(q1t[:, o], q2t[:, o])
        v = v + p * (q - alpha * logp)
    v = v.reshape(M, NA)
    masked = np.zeros(M, bool)
    if mask_dones:
        masked = inp["dones"].astype(bool)
    y = inp["rewards"].astype(f) + discount * np.where(masked[:, None], f(0), v)
    n = np.full(M, NA) if inp.get("n") is None else np.clip(inp["n"].astype(np.int64), 0, NA)
    live = np.arange(NA)[None, :] < n[:, None]
    y = np.where(live, y, f(0)).astype(f)
    if inp.get("q1") is None:
        return y, None, None
    a = inp["actions"].astype(np.int64)
    a = np.where((a >= 0) & (a < 9), a, 4).reshape(rows)
    r = np.arange(rows)
    yr = y.reshape(rows)
    d1 = np.abs(inp["q1"].astype(f)[r, a] - yr)
    if inp.get("q2") is None:
        td_rows = d1
    else:
        td_rows = f(0.5) * (d1 + np.abs(inp["q2"].astype(f)[r, a] - yr))
    td_rows = np.where(live, td_rows.reshape(M, NA), f(0)).astype(f)
    tot = np.zeros(M, f)
    for i in range(NA):
        tot = tot + td_rows[:, i]
    td = np.where(n > 0, tot / np.maximum(n, 1).astype(f), f(0)).astype(f)
    return y, td_rows, td


def bounds(NA, alpha, discount, rmax=10.0, L=L_LOGIT, Qm=QM):
    """(bound of y and td_rows, bound of td)."""
    S = rmax + discount * (Qm + alpha * (2 * L + np.log(9.0)))
    return 64 * EPS24 * S, 2 * (64 + NA) * EPS24 * (S + Qm)


def make_inputs(M, NA, seed):
    """Uniform logits in [-4, 4], Q values in [-10, 10], rewards from {-1, 0, 1, 10}, a third of the
    samples done, actions 0..8 with -3 and 9 planted on live rows, n mixing -1, 0, partial counts
    and NA."""
    rng = np.random.default_rng(seed)
    rows = M * NA
    inp = {k: rng.uniform(-L_LOGIT, L_LOGIT, (rows, 9)).astype(np.float32) for k in ("pi_next",)}
    for k in ("q1t_next", "q2t_next", "q1", "q2"):
        inp[k] = rng.uniform(-QM, QM, (rows, 9)).astype(np.float32)
    inp["actions"] = rng.integers(0, 9, (M, NA)).astype(np.int32)
    inp["rewards"] = REWARDS[rng.integers(0, 4, (M, NA))]
    inp["dones"] = (rng.random(M) < 1 / 3).astype(np.uint8)
    n = rng.choice(np.array([-1, 0, max(1, NA // 2), max(1, NA - 1), NA]), M).astype(np.int32)
    n[0] = NA
    for m, v in ((1, -1), (2, 0), (3, max(1, NA // 2)), (4, NA), (M - 1, NA - 1 if NA > 1 else NA)):
        if 0 < m < M:
            n[m] = v
    inp["n"] = n
    inp["actions"][0, 0] = -3
    inp["actions"][0, NA - 1] = 9 if NA > 1 else -3
    if M > 4:
        inp["actions"][4, 0] = 9
        inp["dones"][4], inp["dones"][0] = 1, 0
    return inp


def peaked_logits(rows, seed):
    """pi_next of a near-deterministic trained policy: one logit of every row at +60 and the rest in
    [-60, 0] (exp underflows to 0 where the distance exceeds 103, logp is near -120); with more than
    one row, row 0 -- always live: n[0] = NA -- holds nine equal logits."""
    rng = np.random.default_rng(seed)
    pi = rng.uniform(-L_PEAKED, 0.0, (rows, 9)).astype(np.float32)
    pi[np.arange(rows), rng.integers(0, 9, rows)] = L_PEAKED
    if rows > 1:
        pi[0] = L_PEAKED
    return pi


# option cases: (name, twin target, q networks: 2 / 1 / 0, use n, mask_dones, alpha, byte offset of every array
# [, the bound L of |pi_next|: L_PEAKED takes peaked_logits])
OPTIONS = (
    ("twin, n, no mask", True, 2, True, 0, 0.2, 0),
    ("twin, n = NULL, mask, alpha 0, offset 4", True, 2, False, 1, 0.0, 4),
    ("single Q, n, mask", False, 1, True, 1, 0.2, 0),
    ("single Q, twin target, offset 4", True, 1, True, 0, 0.2, 4),
    ("targets only, offset 4", True, 0, True, 0, 0.2, 4),
    ("targets only, single target, n = NULL, mask", False, 0, False, 1, 0.2, 0),
    ("peaked policies, twin, n, no mask, offset 4", True, 2, True, 0, 0.2, 4, L_PEAKED),
)


def _place(arr, device, offset):
    """A copy of `arr` at byte `offset` (4: 4-byte but not 16-byte aligned) of a fresh buffer."""
    raw = torch.zeros(arr.nbytes + offset + 16, dtype=torch.uint8, device=device)
    assert raw.data_ptr() % 16 == 0
    raw[offset:offset + arr.nbytes] = torch.as_tensor(np.ascontiguousarray(arr).view(np.uint8).reshape(-1)).to(device)
    return raw


def _guarded(nbytes, device, offset):
    raw = torch.full((offset + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=device)
    assert raw.data_ptr() % 16 == 0
    return raw


def run_td(nat, lib, device, M, NA, inp, *, alpha, discount, mask_dones, offset=0, outputs=("y", "td_rows", "td")):
    """wh_sac_td of one library on `inp` (None entries = NULL); the outputs as numpy, their head and
    guard bytes checked."""
    keep, ptr = {}, {}
    for k in ("pi_next", "q1t_next", "q2t_next", "q1", "q2", "actions", "rewards", "dones", "n"):
        if inp.get(k) is None:
            ptr[k] = None
        else:
            off = offset if inp[k].dtype != np.uint8 else 0
            keep[k] = _place(inp[k], device, off)
            ptr[k] = keep[k].data_ptr() + off
    sizes = dict(y=4 * M * NA, td_rows=4 * M * NA, td=4 * M)
    out = {k: _guarded(sizes[k], device, offset) for k in outputs}
    args = nat.WhSacTdArgs(ptr["pi_next"], ptr["q1t_next"], ptr["q2t_next"], ptr["q1"], ptr["q2"], ptr["actions"],
                           ptr["rewards"], ptr["dones"], ptr["n"], alpha, discount, mask_dones,
                           *[(out[k].data_ptr() + offset) if k in out else None for k in ("y", "td_rows", "td")])
    rc = lib.wh_sac_td(M, NA, ctypes.byref(args), nat.stream_of(torch.device(device)))
    assert rc == nat.WH_OK, rc
    res = {}
    for k, t in out.items():
        h = t.cpu().numpy()
        assert (h[:offset] == 0xA5).all() and (h[offset + sizes[k]:] == 0xA5).all(), f"bytes written outside {k}"
        res[k] = h[offset:offset + sizes[k]].copy().view(np.float32).reshape((M, NA) if k != "td" else (M,))
    return res


def case_td(nat, lib, device, NA, M, quarter=False):
    """Every option case at one (NA, M) against the float64 model, within the stated bounds (a
    quarter of them with `quarter`: what the host engine and the float32 model must keep); exact
    zeros where the contract states them.  Returns the largest errors seen, as fractions of the bounds."""
    inp0 = make_inputs(M, NA, 1000 * NA + M)
    worst = dict(y=0.0, td_rows=0.0, td=0.0)
    for name, twin_t, nq, use_n, mask, alpha, offset, *rest in OPTIONS:
        L = rest[0] if rest else L_LOGIT
        inp = dict(inp0)
        if L == L_PEAKED:
            inp["pi_next"] = peaked_logits(M * NA, 1000 * NA + M)
        assert float(np.abs(inp["pi_next"]).max()) <= L
        if not twin_t:
            inp["q2t_next"] = None
        if nq < 2:
            inp["q2"] = None
        if nq < 1:
            inp["q1"] = None
        if not use_n:
            inp["n"] = None
        if not mask:
            inp = dict(inp, dones=inp["dones"] if offset else None)   # dones may be NULL without the mask
        outputs = ("y", "td_rows", "td") if nq else ("y",)
        got = run_td(nat, lib, device, M, NA, inp, alpha=alpha, discount=DISCOUNT, mask_dones=mask, offset=offset,
                     outputs=outputs)
        want = dict(zip(("y", "td_rows", "td"), model(inp, NA, alpha=alpha, discount=DISCOUNT, mask_dones=mask)))
        by, btd = bounds(NA, alpha, np.float32(DISCOUNT), L=L)
        scale = 0.25 if quarter else 1.0
        for k in outputs:
            err = float(np.abs(got[k].astype(np.float64) - want[k]).max())
            b = btd if k == "td" else by
            key = k if L == L_LOGIT else "peaked " + k
            worst[key] = max(worst.get(key, 0.0), err / b)
            assert err <= scale * b, f"NA={NA} M={M} [{name}] {k}: error {err:.3e}, bound {scale * b:.3e}"
        # exact zeros: rows i >= n[m], everything of samples with n[m] <= 0
        n = np.full(M, NA) if inp["n"] is None else inp["n"]
        dead = np.arange(NA)[None, :] >= np.clip(n, 0, NA)[:, None]
        for k in outputs:
            bits = got[k].view(np.uint32)
            if k == "td":
                assert not bits[n <= 0].any(), f"[{name}] td of samples with n <= 0"
            else:
                assert not bits[dead].any(), f"[{name}] {k} of rows i >= n[m]"
    return worst


def case_float32_model(NA, M):
    """The float32 numpy transcription of the formula stays under a quarter of the bounds on the
    test's own inputs (if it did not, the operation order would be wrong, not the bound)."""
    inp0 = make_inputs(M, NA, 1000 * NA + M)
    worst = dict(y=0.0, td_rows=0.0, td=0.0)
    for alpha, mask, L in ((0.2, 0, L_LOGIT), (0.0, 1, L_LOGIT), (0.2, 0, L_PEAKED)):
        inp = inp0 if L == L_LOGIT else dict(inp0, pi_next=peaked_logits(M * NA, 1000 * NA + M))
        a = model(inp, NA, alpha=alpha, discount=DISCOUNT, mask_dones=mask, dtype=np.float32)
        b = model(inp, NA, alpha=alpha, discount=DISCOUNT, mask_dones=mask)
        by, btd = bounds(NA, alpha, np.float32(DISCOUNT), L=L)
        for k, x, w, bound in zip(("y", "td_rows", "td"), a, b, (by, by, btd)):
            err = float(np.abs(x.astype(np.float64) - w).max())
            key = k if L == L_LOGIT else "peaked " + k
            worst[key] = max(worst.get(key, 0.0), err / bound)
            assert err <= 0.25 * bound, f"float32 model NA={NA} M={M} L={L} {k}: {err:.3e} > {0.25 * bound:.3e}"
    return worst


# ----------------------------------------------------------------------------- refusals
def case_refusals(nat, lib, host: bool):
    """The refusals of wh_sac_td (codes of one library as a list, compared between the libraries by
    the caller).  On the host engine every pointer is a real sentinel-filled buffer that must stay
    untouched; on the device library dummies a refused or empty call never dereferences."""
    M, NA = 3, 4
    keep = []

    def mem(nbytes):
        if not host:
            keep.append(None)
            return 4096 * len(keep)
        t = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8)
        keep.append(t)
        return t.data_ptr()

    rows = M * NA
    base = dict(pi_next=mem(36 * rows), q1t_next=mem(36 * rows), q2t_next=mem(36 * rows), q1=mem(36 * rows),
                q2=mem(36 * rows), actions=mem(4 * rows), rewards=mem(4 * rows), dones=mem(M), n=mem(4 * M),
                alpha=0.2, discount=0.99, mask_dones=0, y=mem(4 * rows), td_rows=mem(4 * rows), td=mem(4 * M))

    def call(M_=M, NA_=NA, null_args=False, **over):
        a = dict(base, **over)
        return lib.wh_sac_td(M_, NA_, None if null_args else ctypes.byref(nat.WhSacTdArgs(**a)), None)

    E, OK = nat.WH_EINVAL, nat.WH_OK
    table = [
        ("NULL args", call(null_args=True), E),
        ("NULL args, M = 0", call(M_=0, null_args=True), E),
        ("M -1", call(M_=-1), E),
        ("NA 0", call(NA_=0), E),
        ("NA -2", call(NA_=-2), E),
        ("NA 17", call(NA_=17), E),
        ("NA 17, M = 0", call(M_=0, NA_=17), E),
        ("no output", call(y=None, td_rows=None, td=None), E),
        ("NULL pi_next", call(pi_next=None), E),
        ("NULL q1t_next", call(q1t_next=None), E),
        ("NULL actions", call(actions=None), E),
        ("NULL rewards", call(rewards=None), E),
        ("td_rows without q1", call(q1=None, q2=None, td=None), E),
        ("td without q1", call(q1=None, q2=None, td_rows=None), E),
        ("q2 without q1", call(q1=None, td_rows=None, td=None), E),
        ("mask_dones without dones", call(mask_dones=1, dones=None), E),
        ("M = 0", call(M_=0), OK),
        ("M = 0, NULL arrays", call(M_=0, **{k: None for k in base if k not in ("alpha", "discount", "mask_dones")}), OK),
    ]
    for what, rc, want in table:
        assert rc == want, f"{what}: got {rc}, expected {want}"
    for t in keep:
        assert t is None or bool((t == 0xA5).all()), "a refused (or empty) call wrote to a buffer"
    return [(what, rc) for what, rc, _ in table]


# ----------------------------------------------------------------------------- pack (device only)
VARIANT_DIMS = {"small": (37, 256, 256), "medium": (82, 512, 512), "large": (145, 1024, 256)}


def pack_weights(in_dim, h0, h1, seed):
    """Random weights with planted values: bf16 rounding ties in both directions, roundings that
    carry into the exponent, -0.0, f32 denormals, +-3e38, and b0 entries whose hi/lo split is
    inexact in one bf16."""
    rng = np.random.default_rng(seed)
    w = {}
    for k, shp in (("w0", (h0, in_dim)), ("b0", (h0,)), ("w1", (h1, h0)), ("b1", (h1,)), ("w2", (9, h1)), ("b2", (9,))):
        w[k] = rng.uniform(-1.0, 1.0, shp).astype(np.float32)
    bits = np.array([0x3FFFFFFF, 0xBFFFFFFF, 0x3F7FFFFF, 0x40FFC000, 0x3F808000, 0x3F818000], np.uint32).view(np.float32)
    special = np.concatenate([
        np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 2.0 ** -8 + 2.0 ** -16,
                  -0.0, 0.0, 1e-40, -1e-41, 1.4e-45, 3e38, -3e38, 1 + 2.0 ** -8 + 2.0 ** -20, 1 + 2.0 ** -8 - 2.0 ** -20],
                 np.float32), bits])
    assert np.signbit(special[5]) and special[7] != 0 and abs(special[7]) < 1.2e-38
    for k in ("w0", "w1", "w2", "b1"):
        flat = w[k].reshape(-1)
        pos = rng.choice(flat.size, len(special), replace=False)
        flat[pos] = special
        flat[:3] = special[:3]                    # ... and at the first elements
        flat[-2:] = special[10:12]                # +-3e38 at the last
    # b0 = hi + lo: values one bf16 cannot hold (the lo part matters), a denormal, a tie, a huge one
    w["b0"][:10] = np.array([0.1, -1 / 3, 1 + 2.0 ** -10, 1 + 2.0 ** -8, 1e-40, -0.0, 3e38, 123.456, -2.0 ** -100, 1.99999988],
                            np.float32)
    w["b2"][:3] = special[:3]
    return w


def case_pack_equal(nat, variant, precision, seed=0):
    """wh_mlp_pack_device's blob equals wh_mlp_pack's from the same values, byte for byte: exactly
    wh_mlp_query bytes each, with a sentinel guard behind both that survives."""
    dev = torch.device("cuda:0")
    in_dim, h0, h1 = VARIANT_DIMS[variant]
    desc = nat.WhMlpDesc(in_dim, h0, h1, 9, {"bf16": nat.WH_MLP_BF16, "f32": nat.WH_MLP_F32}[precision])
    nbytes = ctypes.c_int64()
    assert nat.lib().wh_mlp_query(ctypes.byref(desc), ctypes.byref(nbytes)) == nat.WH_OK
    nb = int(nbytes.value)
    w = pack_weights(in_dim, h0, h1, seed)
    keys = ("w0", "b0", "w1", "b1", "w2", "b2")
    fp = ctypes.POINTER(ctypes.c_float)
    host_blob = torch.full((nb + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    dev_blob = torch.full((nb + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = nat.lib().wh_mlp_pack(ctypes.byref(desc), *[w[k].ctypes.data_as(fp) for k in keys], host_blob.data_ptr())
    assert rc == nat.WH_OK, rc
    wd = {k: torch.as_tensor(w[k]).to(dev).contiguous() for k in keys}
    rc = nat.lib().wh_mlp_pack_device(ctypes.byref(desc), *[wd[k].data_ptr() for k in keys], dev_blob.data_ptr(),
                                      nat.stream_of(dev))
    assert rc == nat.WH_OK, rc
    torch.cuda.synchronize(dev)
    assert bool((host_blob[nb:] == 0xA5).all()) and bool((dev_blob[nb:] == 0xA5).all()), "bytes written past the blob"
    assert torch.equal(dev_blob[:nb], host_blob[:nb]), f"{variant} {precision}: device and host blobs differ"
    return nb


if __name__ == "__main__":   # the WH_MLP_LEGACY child of tests/test_gpu_sac.py: bf16 Medium on the 32x32x16 route
    import os
    import sys

    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [ROOT, os.path.join(ROOT, "rllib-warehouse_amd")]
    from warehouse import _native

    assert os.environ.get("WH_MLP_LEGACY") == "1"
    print("LEGACY PACK OK", case_pack_equal(_native, "medium", "bf16", seed=5))
