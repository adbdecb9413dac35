"""Test bodies of wh_adam_step (csrc/adam.h, csrc/sac_formula.h; include/warehouse_amd.h, ADAM).

tests/test_adam_cpu.py holds the host engine to the float64 model of the formula and to torch.optim.Adam;
tests/test_gpu_adam.py holds the device to the host engine bit for bit.  Everything goes through the C ABI
on guarded buffers: 0xA5 before and behind every tensor.

Bounds of the host engine against the float64 model (each f32 operation rounds by at most 2^-24 relative;
D = step_size m' / denom is the step, A = |beta1 m| + |omb1 g| bounds what m' is made of):
  m'   3 * 2^-24 * A                two products and a sum
  v'   4 * 2^-24 * v'               three products and a sum of non-negative terms
  p'   step_size / denom * 3 * 2^-24 * A  (the error of m' carried through)  +  8 * 2^-24 |D|  (sqrt, two
       divisions, the sum with eps, the product, and v' entering under a square root)  +  2^-24 |p|  (the
       final subtraction)
torch.optim.Adam is held to 4 x these (its lerp form of m' rounds up to 1.22 x ours; the rest is the same
mathematics).  An element whose (omb2 g) g overflows f32 -- the planted g = 1e30 -- is outside the model:
there v' = inf and the step is 0 on every engine, which is asserted instead.
"""
import ctypes

import numpy as np
import torch

GUARD = 256
EPS24 = 2.0 ** -24
LR, BETAS, EPS = 3e-4, (0.9, 0.999), 1e-8
# (count, byte offset of p / m / v, byte offset of g): 24 segments -- the issue's counts, the chunk edges of
# k_adam (2,048 elements a workgroup), one segment with all four pointers at offset 4, one with g alone
SEGMENTS = ((0, 0, 0), (1, 0, 0), (3, 0, 0), (4, 0, 0), (5, 0, 0), (4095, 0, 0), (4096, 0, 0), (4097, 0, 0),
            (300000, 0, 0), (2049, 4, 4), (2047, 0, 4), (2048, 0, 0), (7, 4, 4), (0, 4, 4), (513, 0, 0), (9, 0, 0),
            (1025, 0, 4), (64, 0, 0), (255, 0, 0), (257, 0, 0), (2, 0, 0), (6, 0, 8), (8191, 0, 0), (1, 4, 4))
assert len(SEGMENTS) == 24


def make_state(seed, segments=SEGMENTS):
    """p, m, g from seeded normals and v = normal^2, with planted values where a segment has room: g of
    0, -0, 1e-30, 1e30 at elements 0..3 (v = 0 beside the g of 0), p of 1e30 / 1e-30 / 0 / -0 at 0..3."""
    rng = np.random.default_rng(seed)
    st = []
    for count, _, _ in segments:
        p, m, g = (rng.standard_normal(count).astype(np.float32) for _ in range(3))
        v = (rng.standard_normal(count).astype(np.float32) ** 2 * np.float32(0.01)).astype(np.float32)
        plant_gradients(g)
        p[:4] = np.array([1e30, 1e-30, 0.0, -0.0], np.float32)[:min(4, count)]
        if count:
            v[0] = 0.0
        st.append(dict(p=p, m=m, v=v, g=g))
    return st


def plant_gradients(g):
    g[:4] = np.array([0.0, -0.0, 1e-30, 1e30], np.float32)[:min(4, g.size)]


def fresh_gradients(seed, segments=SEGMENTS):
    rng = np.random.default_rng(seed)
    out = []
    for count, _, _ in segments:
        g = rng.standard_normal(count).astype(np.float32)
        plant_gradients(g)
        out.append(g)
    return out


class Run:
    """The state of `segments` in guarded buffers of one engine ("cpu": the host engine)."""

    def __init__(self, nat, lib, device, state, segments=SEGMENTS):
        self.nat, self.lib, self.device, self.segments = nat, lib, device, segments
        self.buf = []
        for (count, off, goff), st in zip(segments, state):
            b = {}
            for k in ("p", "m", "v", "g"):
                o = goff if k == "g" else off
                raw = torch.full((GUARD + o + 4 * count + GUARD,), 0xA5, dtype=torch.uint8, device=device)
                assert raw.data_ptr() % 16 == 0
                b[k] = (raw, GUARD + o)
            self.buf.append(b)
        self.put(state, ("p", "m", "v", "g"))

    def put(self, state, keys):
        for (count, _, _), b, st in zip(self.segments, self.buf, state):
            for k in keys:
                raw, o = b[k]
                raw[o:o + 4 * count] = torch.as_tensor(np.ascontiguousarray(st[k]).view(np.uint8)).to(self.device)

    def step(self, t, lr=LR, betas=BETAS, eps=EPS, nseg=None):
        nat = self.nat
        n = len(self.segments) if nseg is None else nseg
        arr = (nat.WhAdamSeg * max(1, n))()
        for i in range(n):
            b = self.buf[i]
            arr[i] = nat.WhAdamSeg(*[b[k][0].data_ptr() + b[k][1] for k in ("p", "m", "v", "g")], self.segments[i][0])
        h = nat.adam_hyper(lr, betas[0], betas[1], eps, t)
        rc = self.lib.wh_adam_step(n, arr, ctypes.byref(h), nat.stream_of(torch.device(self.device)))
        assert rc == nat.WH_OK, rc
        return h

    def get(self):
        """[{p, m, v}] as numpy; every guard (g's too) checked."""
        out = []
        for (count, _, _), b in zip(self.segments, self.buf):
            d = {}
            for k in ("p", "m", "v", "g"):
                raw, o = b[k]
                h = raw.cpu().numpy()
                assert (h[:o] == 0xA5).all() and (h[o + 4 * count:] == 0xA5).all(), f"bytes written outside {k}"
                d[k] = h[o:o + 4 * count].copy().view(np.float32)
            out.append(d)
        return out


def model_bounds(st, h):
    """float64 model of one step from state `st` (one segment) and hyper `h`, with the bounds of the
    module docstring: (p', m', v', bound p, bound m, bound v, mask of the elements inside the model)."""
    f = np.float64
    b1, o1, b2, o2, eps, ss, bc2 = (f(getattr(h, k)) for k in ("beta1", "omb1", "beta2", "omb2", "eps", "step_size",
                                                                "sqrt_bc2"))
    p, m, v, g = (st[k].astype(f) for k in ("p", "m", "v", "g"))
    m1 = b1 * m + o1 * g
    v1 = b2 * v + (o2 * g) * g
    denom = np.sqrt(v1) / bc2 + eps
    D = ss * (m1 / denom)
    A = np.abs(b1 * m) + np.abs(o1 * g)
    bm = 3 * EPS24 * A
    bv = 4 * EPS24 * v1
    bp = ss / denom * bm + 8 * EPS24 * np.abs(D) + EPS24 * np.abs(p)
    inside = (o2 * g) * g < f(np.finfo(np.float32).max)
    return p - D, m1, v1, bp, bm, bv, inside


def case_host_against_model(nat, t, seed=0):
    """One host-engine step at step count t against the float64 model and one torch.optim.Adam step from
    the same state (within 4 x the bounds).  Returns the largest error / bound ratios."""
    state = make_state(seed + t)
    run = Run(nat, nat.host_lib(), "cpu", state)
    h = run.step(t)
    got = run.get()
    worst = {}
    for (count, _, _), st, out in zip(SEGMENTS, state, got):
        assert np.array_equal(out["g"].view(np.uint32), st["g"].view(np.uint32))
        if not count:
            continue
        p1, m1, v1, bp, bm, bv, inside = model_bounds(st, h)
        # torch from the same state: its state's step is t - 1 before the call
        tp = torch.nn.Parameter(torch.as_tensor(st["p"].copy()))
        opt = torch.optim.Adam([tp], lr=LR, betas=BETAS, eps=EPS)
        opt.state[tp] = dict(step=torch.tensor(float(t - 1)), exp_avg=torch.as_tensor(st["m"].copy()),
                             exp_avg_sq=torch.as_tensor(st["v"].copy()))
        tp.grad = torch.as_tensor(st["g"].copy())
        opt.step()
        ref = dict(p=tp.detach().numpy(), m=opt.state[tp]["exp_avg"].numpy(), v=opt.state[tp]["exp_avg_sq"].numpy())
        for k, want, bound in (("p", p1, bp), ("m", m1, bm), ("v", v1, bv)):
            err = np.abs(out[k].astype(np.float64)[inside] - want[inside])
            ok = err <= bound[inside]
            assert ok.all(), f"t={t} count={count} {k}: error {err[~ok].max():.3e} over its bound"
            terr = np.abs(ref[k].astype(np.float64)[inside] - out[k].astype(np.float64)[inside])
            tok = terr <= 4 * bound[inside]
            assert tok.all(), f"t={t} count={count} torch {k}: {terr[~tok].max():.3e} over 4 x the bound"
            nz = bound[inside] > 0
            if nz.any():
                worst[k] = max(worst.get(k, 0.0), float((err[nz] / bound[inside][nz]).max()))
                worst["torch " + k] = max(worst.get("torch " + k, 0.0), float((terr[nz] / (4 * bound[inside][nz])).max()))
        over = ~inside                                  # g = 1e30: v' overflows, the step is 0
        assert np.isinf(out["v"][over]).all() and np.array_equal(out["p"][over], st["p"][over])
        assert np.isinf(ref["v"][over]).all() and np.array_equal(ref["p"][over], st["p"][over])
        assert over.sum() == (1 if count >= 4 else 0)
    return worst


def case_device_equals_host(nat, t0, steps, seed=0):
    """`steps` chained calls from step count t0 with fresh gradients each, on the device and on the host
    engine: p, m, v equal bit for bit after every call."""
    state = make_state(seed + t0)
    dev = Run(nat, nat.lib(), "cuda:0", state)
    host = Run(nat, nat.host_lib(), "cpu", state)
    for k in range(steps):
        if k:
            g = [dict(g=x) for x in fresh_gradients(seed + 100 * t0 + k)]
            dev.put(g, ("g",))
            host.put(g, ("g",))
        dev.step(t0 + k)
        host.step(t0 + k)
        if k in (0, steps - 1):
            a, b = dev.get(), host.get()
            for (count, off, goff), x, y in zip(SEGMENTS, a, b):
                for key in ("p", "m", "v"):
                    same = x[key].view(np.uint32) == y[key].view(np.uint32)
                    assert same.all(), (f"call {k + 1} from t={t0}, segment of {count} at offsets {off}/{goff}: {key} "
                                        f"differs at {np.flatnonzero(~same)[:4]}")


def case_fewer_segments(nat, lib, device):
    """nseg below the table's length touches only the first nseg segments."""
    state = make_state(9)
    run = Run(nat, lib, device, state)
    run.step(3, nseg=5)
    for i, (st, out) in enumerate(zip(state, run.get())):
        changed = not np.array_equal(out["m"].view(np.uint32), st["m"].view(np.uint32))
        assert changed == (i < 5 and SEGMENTS[i][0] > 0), i


# ----------------------------------------------------------------------------- refusals
def case_refusals(nat, lib, host: bool):
    """The refusals of wh_adam_step (codes of one library as a list).  On the host engine every pointer is
    a real sentinel-filled buffer that must stay untouched; on the device library dummies."""
    keep = []

    def mem(nbytes):
        if not host:
            keep.append(None)
            return 4096 * len(keep)
        t = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8)
        assert t.data_ptr() % 16 == 0
        keep.append(t)
        return t.data_ptr()

    count = 6
    good = [mem(4 * count) for _ in range(4)]
    h = nat.adam_hyper(LR, BETAS[0], BETAS[1], EPS, 1)

    def call(nseg=2, null_h=False, null_segs=False, second=None):
        arr = (nat.WhAdamSeg * 25)()
        for i in range(25):
            arr[i] = nat.WhAdamSeg(*good, 0)          # (empty: touches nothing)
        if second is not None:
            arr[1] = nat.WhAdamSeg(*second)
        return lib.wh_adam_step(nseg, None if null_segs else arr, None if null_h else ctypes.byref(h), None)

    def with_ptr(i, v):
        s = list(good) + [count]
        s[i] = v
        return s

    E, OK = nat.WH_EINVAL, nat.WH_OK
    table = [("nseg -1", call(nseg=-1), E), ("nseg 25", call(nseg=25), E), ("NULL h", call(null_h=True), E),
             ("NULL h, nseg 0", call(nseg=0, null_h=True), E), ("NULL segs", call(null_segs=True), E),
             ("count -1", call(second=list(good) + [-1]), E)]
    for i, k in enumerate(("p", "m", "v", "g")):
        table.append((f"NULL {k}", call(second=with_ptr(i, None)), E))
        for o in (1, 2, 3):
            table.append((f"{k} at offset {o}", call(second=with_ptr(i, good[i] + o)), E))
    table += [("nseg 0", call(nseg=0), OK), ("nseg 0, NULL segs", call(nseg=0, null_segs=True), OK),
              ("24 empty segments", call(nseg=24), OK),
              ("count 0 with NULL pointers", call(second=[None, None, None, None, 0]), OK)]
    for what, rc, want in table:
        assert rc == want, f"{what}: got {rc}, expected {want}"
    for t in keep:
        assert t is None or bool((t == 0xA5).all()), "a refused (or empty) call wrote to a buffer"
    return [(what, rc) for what, rc, _ in table]
