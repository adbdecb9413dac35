"""Integer-valued policy networks on which the MLP kernels (k_mlp, k_mlp16, k_mlp_f32; csrc/mlp32.h,
mlp16.h, mlp_f32.h, fed by the three maps of csrc/mlp_pack.h) must give EXACT answers: the generator, a
plain numpy float64 reference, and the GPU bodies shared by tests/test_gpu_mlp_exact.py and its
WH_MLP_LEGACY child process (this file run as a program).  tests/test_mlp_exact_cpu.py checks, without
a GPU, the conditions that make the GPU comparison mean something.

Why tolerance 0 is right.  Every weight, bias and input is a small integer (one planted input row also
holds multiples of 2^-2), and for every row the sum  sum_k |w||h| + |b|  of every dot product, counted
in the row's grain (1, or 2^-2 for that row), stays below 2^24.  Then every bf16 x bf16 product and
every partial sum, in any order and any fusing, is exactly representable in f32, the bf16 rounding of a
hidden unit is a function of an exact value, and the nine logits are exact.  The kernel has no freedom
left: one misplaced weight, a truncating or wrongly tie-breaking rounding, a lost `lo` half of b0
changes some logit by at least one grain, and the comparison fails.

Value ranges are those of the issue that asked for these tests, with these changes made to meet its own
conditions (tests/test_mlp_exact_cpu.py holds all of them):
  * b0 plants four more entries that one bf16 cannot hold (259, -257, 513, -1025) behind the issue's
    eight: of those only six have lo != 0 (300 and -33 are exact in bf16), and eight are asked for.
  * The planted rounding row holds +-257, +-259 and, in place of +-(1 + 2^-8) and +-(1 + 3 2^-8), the
    same significands 64 times larger: +-64.25 and +-64.75 (ties to 64 and to 65: both directions).  On
    the f32 kernel, which rounds nothing, the row's grain travels through all three layers, and the
    row's layer-2 sum on Medium is 1.4e6 (its inputs are the largest): 3.6e8 grains of 2^-8, over the
    limit of 2^24 = 1.7e7, and 5.7e6 grains of 2^-2.
  * b1 is 4 x integers in [-64, 64] minus what the planted b0 alone send into the unit (w1 times their
    positive values, rounded to a multiple of 4).  Without that the planted units, whose activation is
    about 1,000 in every row, decide most of layer 1 on their own: 21 of Small's 256 and 25 of Medium's
    512 layer-1 units were dead in all 300 rows, so nothing in their rows of W1 could show, and only
    197 of 200 swaps in Small's W1 were seen.  With it at most 2 units are dead in every row.
  * The seeds are chosen per variant (SEED) so that the 300-row case meets the coverage conditions:
    with many seeds the tied pair is the maximum in fewer than 20 rows.

Layout of inputs(variant, seed, rows): row rows // 3 is the rounding row, the last row is all zeros
(rows > 1), rows with index % 4 == 1 hold only 0 / 1 (the special rows win where they collide).
Coverage and sensitivity are properties of the 300-row case of every variant; exactness,
representability and order independence hold for every case the GPU test runs (CASES)."""
import numpy as np

VARIANT_DIMS = {"small": (37, 256, 256), "medium": (82, 512, 512), "large": (145, 1024, 256)}
VARIANTS = tuple(VARIANT_DIMS)
ROWS = (1, 31, 33, 255, 257, 300)        # one row, the 32-row tile edge, the 256-row task edge, a ragged tail
SEED = {"small": 8, "medium": 2, "large": 11}     # the one-network cases (module docstring)
MANY = ((21, 33), (22, 257), (23, 1))    # forward_many: (seed, rows) of its three jobs
B0_PLANTED = (257, -259, 1027, -515, 300, 387, -33, 641, 259, -257, 513, -1025)
TIED = (2, 6)                            # the two identical rows of w2 (equal b2): logits 2 and 6 tie in every row
INT_ROUNDED = (257.0, 259.0, -257.0, -259.0)
FRAC_ROUNDED = (64.25, 64.75, -64.25, -64.75)
LIMIT = 2.0 ** 24
KEYS = ("w0", "b0", "w1", "b1", "w2", "b2")
# every (variant, seed, rows) the GPU test computes a reference for
CASES = tuple((v, SEED[v], r) for v in VARIANTS for r in ROWS) + tuple((v, s, r) for v in VARIANTS for s, r in MANY)


# ----------------------------------------------------------------------------- bf16, in integer code
def bf16_bits(a):
    """The bf16 bit patterns (uint16) of float32 values, round to nearest, ties to even."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = u + 0x7FFF + ((u >> 16) & 1)
    return ((u >> 16) & 0xFFFF).astype(np.uint16)


def to_bf16(a):
    """Float32 values rounded to bf16 (nearest, ties to even), as float32."""
    return (bf16_bits(a).astype(np.uint32) << 16).view(np.float32)


def trunc_bf16(a):
    """The wrong rounding of mutation tests: the low 16 bits dropped."""
    return (np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def away_bf16(a):
    """The wrong rounding of mutation tests: nearest, ties away from zero."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64) + 0x8000
    return ((u >> 16 << 16) & 0xFFFFFFFF).astype(np.uint32).view(np.float32)


def ties(pre):
    """(rounded down to even, rounded up to even): how many live values of `pre` (exact in f32) lie
    exactly between two bf16 neighbours."""
    u = np.ascontiguousarray(pre, dtype=np.float32).view(np.uint32)
    tie = (pre > 0) & ((u & 0xFFFF) == 0x8000)
    odd = ((u >> 16) & 1).astype(bool)
    return int((tie & ~odd).sum()), int((tie & odd).sum())


# ----------------------------------------------------------------------------- the generator
def network(variant, seed):
    """The six float32 arrays (nn.Linear layout) of an integer-valued network."""
    in_dim, h0, h1 = VARIANT_DIMS[variant]
    rng = np.random.default_rng([seed, VARIANTS.index(variant), 1])
    w0 = rng.choice(np.array([-3, -2, -1, 1, 2, 3]), (h0, in_dim)) * (rng.random((h0, in_dim)) < 0.5)
    b0 = rng.integers(-40, 41, h0)
    b0[:len(B0_PLANTED)] = B0_PLANTED
    w1 = rng.choice(np.array([-2, -1, 1, 2]), (h1, h0)) * (rng.random((h1, h0)) < 24.0 / h0)
    b1 = 4 * rng.integers(-64, 65, h1)
    b1 -= 4 * np.round(w1[:, :len(B0_PLANTED)] @ np.maximum(B0_PLANTED, 0) / 4).astype(b1.dtype)   # module docstring
    w2 = rng.choice(np.array([-1, 1]), (9, h1))
    b2 = rng.integers(-8, 9, 9)
    w2[TIED[1]] = w2[TIED[0]]
    b2[TIED[1]] = b2[TIED[0]]
    w = dict(w0=w0, b0=b0, w1=w1, b1=b1, w2=w2, b2=b2)
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in w.items()}


def inputs(variant, seed, rows):
    """[rows, IN] float32 (module docstring: layout)."""
    in_dim = VARIANT_DIMS[variant][0]
    rng = np.random.default_rng([seed, VARIANTS.index(variant), 2, rows])
    x = rng.integers(-9, 10, (rows, in_dim)).astype(np.float32)
    binary = rng.integers(0, 2, (rows, in_dim)).astype(np.float32)
    x[1::4] = binary[1::4]
    if rows > 1:
        x[rows - 1] = 0
    x[rounding_row(rows), rng.choice(in_dim, 16, replace=False)] = np.tile(np.array(INT_ROUNDED + FRAC_ROUNDED, np.float32), 2)
    return x


def rounding_row(rows):
    """The index of the row that holds the values bf16 cannot hold."""
    return rows // 3


def grain(x):
    """Per row, the power of two that every value of the row (and so of everything computed from it
    with integer weights) is a multiple of: 2^-2 for a row with a fraction, else 1."""
    assert np.array_equal(4 * x, np.round(4 * x))
    return np.where((x != np.round(x)).any(axis=1), 0.25, 1.0)


# ----------------------------------------------------------------------------- the reference
def split_b0(b0):
    """b0 as the bf16 pair the packer stores in the two spare k columns of W0."""
    hi = to_bf16(b0)
    return hi, to_bf16(b0 - hi)


def reference(w, x, precision, *, hidden=to_bf16, xround=to_bf16, drop_lo=False):
    """The network in float64 on exactly representable values.  "bf16": x rounded, b0 as hi + lo,
    each hidden layer hidden(max(pre, 0)); "f32": nothing rounded.  Returns a dict: logits [rows, 9]
    float64, actions (first maximum), h0 / h1 / h2 (every layer's input), pre0 / pre1 (before ReLU),
    b0 (as it entered), worst (per layer, the largest sum |w||h| + |b| in grains of its row).
    hidden / xround / drop_lo are the mutation tests' wrong variants."""
    f = np.float64
    bf = precision == "bf16"
    assert precision in ("bf16", "f32")
    g = grain(x)[:, None]
    x = np.asarray(x, np.float32)
    h = (xround(x) if bf else x).astype(f)
    W = {k: v.astype(f) for k, v in w.items()}
    if bf:
        hi, lo = split_b0(w["b0"])
        b0, b0abs = hi.astype(f) + (0 if drop_lo else lo.astype(f)), np.abs(hi).astype(f) + np.abs(lo)
    else:
        b0, b0abs = W["b0"], np.abs(W["b0"])
    out, worst = dict(b0=b0), []
    for i, (b, babs) in enumerate(((b0, b0abs), (W["b1"], np.abs(W["b1"])), (W["b2"], np.abs(W["b2"])))):
        wi = W[f"w{i}"]
        out[f"h{i}"] = h                              # layer i's input
        worst.append(float(((np.abs(h) @ np.abs(wi).T + babs) / g).max()))
        pre = h @ wi.T + b
        if i == 2:
            out["logits"] = pre
            break
        out[f"pre{i}"] = pre
        h = np.maximum(pre, 0)
        if bf:
            assert np.array_equal(h.astype(np.float32).astype(f), h), "a hidden value is not exact in f32"
            h = hidden(h.astype(np.float32)).astype(f)
    out["actions"] = first_max(out["logits"])
    out["worst"] = worst
    return out


def logits_with(w, ref, k, m):
    """The bf16 reference's logits with matrix `k` replaced by `m`, which differs from w[k] in a few
    rows only: the units of those rows are computed again and the later layers follow (all float64 on
    exact values, so the result is reference()'s)."""
    f = np.float64
    units = np.flatnonzero((m != w[k]).any(axis=1))
    act = lambda pre: to_bf16(np.maximum(pre, 0).astype(np.float32)).astype(f)   # noqa: E731
    if k == "w2":
        return ref["h2"] @ m.astype(f).T + w["b2"].astype(f)
    pre1 = ref["pre1"].copy()
    if k == "w1":
        pre1[:, units] = ref["h1"] @ m[units].astype(f).T + w["b1"][units].astype(f)
    else:
        assert k == "w0"
        h1 = act(ref["h0"] @ m[units].astype(f).T + ref["b0"][units])
        pre1 += (h1 - ref["h1"][:, units]) @ w["w1"][:, units].astype(f).T
    return act(pre1) @ w["w2"].astype(f).T + w["b2"].astype(f)


def first_max(z):
    """The index of the first maximum of every row, in plain code (what emit_row does)."""
    best = np.full(z.shape[0], -np.inf)
    arg = np.zeros(z.shape[0], np.int32)
    for o in range(z.shape[1]):
        better = z[:, o] > best
        best = np.where(better, z[:, o], best)
        arg = np.where(better, o, arg).astype(np.int32)
    return arg


def shuffled_f32(w, x, precision, seed):
    """The same network in float32, every dot product accumulated one k at a time in a shuffled order
    (the bias at a random place of it): under the exactness condition the order cannot matter."""
    rng = np.random.default_rng(seed)
    bf = precision == "bf16"
    h = to_bf16(x) if bf else np.asarray(x, np.float32)
    for i in range(3):
        wi, b = w[f"w{i}"], w[f"b{i}"]
        terms = [(wi[:, k], k) for k in range(wi.shape[1])]
        if bf and i == 0:
            hi, lo = split_b0(b)
            terms += [(hi, None), (lo, None)]
        else:
            terms += [(b, None)]
        acc = np.zeros((h.shape[0], wi.shape[0]), np.float32)
        for t in rng.permutation(len(terms)):
            col, k = terms[t]
            acc += col[None, :] if k is None else h[:, k:k + 1] * col[None, :]
        if i == 2:
            return acc
        h = np.maximum(acc, np.float32(0))
        if bf:
            h = to_bf16(h)


def fragments(x, in_dim):
    """The [tiles, kq, 64, 8] bf16 fragment image (uint16 bits) of rows, as wh_observe_x writes it:
    lane 32 h + r of k-step q holds columns 16 q + 8 h .. + 7 of row r of the tile; the two columns
    behind the row are the bias columns 1.0, everything else is padding 0."""
    rows = x.shape[0]
    kq = (in_dim + 2 + 15) // 16
    tiles = (rows + 31) // 32
    full = np.zeros((tiles * 32, 16 * kq), np.float32)
    full[:rows, :in_dim] = x
    full[:, in_dim:in_dim + 2] = 1.0
    bits = bf16_bits(full).reshape(tiles, 32, kq, 2, 8)          # [tile, r, q, h, j]
    return np.ascontiguousarray(bits.transpose(0, 2, 3, 1, 4).reshape(tiles, kq, 64, 8))


# ----------------------------------------------------------------------------- GPU bodies
_refs = {}


def case(variant, seed, rows, precision):
    """(weights, inputs, reference) of one case, computed once and shared (never written)."""
    key = (variant, seed, rows, precision)
    if key not in _refs:
        w, x = network(variant, seed), inputs(variant, seed, rows)
        for a in list(w.values()) + [x]:
            a.setflags(write=False)
        _refs[key] = (w, x, reference(w, x, precision))
    return _refs[key]


def make_net(wh, variant, seed, precision, packer):
    """The network of `seed` on the device, packed by the host packer (the constructor) or by
    wh_mlp_pack_device (load_weights with device tensors, over another network's blob)."""
    import torch

    w = network(variant, seed)
    if packer == "host":
        return wh.policy.MLPPolicy(variant, weights=w, precision=precision)
    assert packer == "device"
    net = wh.policy.MLPPolicy(variant, seed=99, precision=precision)
    net.load_weights({k: torch.as_tensor(w[k]).to(net.device).contiguous() for k in KEYS})
    assert net.weights is None, "load_weights did not take the device packer"
    return net


def check(what, logits, actions, ref, pick=None):
    """Tolerance 0: the logits equal the reference's as values (no NaN), the actions its first maxima."""
    want_l, want_a = ref["logits"], ref["actions"]
    if logits is not None:
        got = logits.cpu().numpy().astype(np.float64)
        got = got if pick is None else got[pick]
        assert got.shape == want_l.shape, (what, got.shape)
        assert not np.isnan(got).any(), f"{what}: NaN logits"
        if not np.array_equal(got, want_l):
            bad = np.argwhere(got != want_l)
            r, o = bad[0]
            raise AssertionError(f"{what}: {len(bad)} of {got.size} logits differ, first at row {r} logit {o}: "
                                 f"kernel {got[r, o]!r}, reference {want_l[r, o]!r}; largest |d| "
                                 f"{np.abs(got - want_l).max()!r} at |ref| up to {np.abs(want_l).max()!r}")
    if actions is not None:
        got = actions.cpu().numpy()
        got = got if pick is None else got[pick]
        if not np.array_equal(got, want_a):
            r = int(np.flatnonzero(got != want_a)[0])
            raise AssertionError(f"{what}: {int((got != want_a).sum())} actions differ, first at row {r}: kernel "
                                 f"{got[r]}, reference {want_a[r]} (logits {want_l[r]})")


def run_entry_points(net, variant, rows, precision):
    """net(x, logits=True), the actions-only launch and (bf16) forward_x on the fragment image of the
    same rows, each against the reference."""
    import torch

    w, x, ref = case(variant, SEED[variant], rows, precision)
    what = f"{variant} {precision} rows {rows}"
    xd = torch.as_tensor(x.copy()).to(net.device).contiguous()
    acts, lg = net(xd, logits=True)
    check(what + " forward", lg, acts, ref)
    acts, none = net(xd)
    assert none is None
    check(what + " actions only", None, acts, ref)
    if precision == "bf16":
        xf = torch.as_tensor(fragments(x, net.in_dim).view(np.int16)).to(net.device).view(torch.uint8).contiguous()
        acts, lg = net.forward_x(xf, rows, logits=True)
        check(what + " forward_x", lg, acts, ref)
        acts, none = net.forward_x(xf, rows)
        assert none is None
        check(what + " forward_x actions only", None, acts, ref)
    tied = (ref["logits"].max(axis=1) == ref["logits"][:, TIED[0]])
    return int(tied.sum())


def run_many(wh, variant, precision):
    """Three seeds' networks with 33, 257 and 1 rows in one forward_many launch; on bf16 the middle
    job reads the fragment operand."""
    import torch

    jobs, refs = [], []
    for i, (seed, rows) in enumerate(MANY):
        w, x, ref = case(variant, seed, rows, precision)
        net = make_net(wh, variant, seed, precision, "host")
        if precision == "bf16" and i == 1:
            xf = torch.as_tensor(fragments(x, net.in_dim).view(np.int16)).to(net.device).view(torch.uint8).contiguous()
            jobs.append(dict(net=net, xfrag=xf, rows=rows, logits=True, actions=True, step=0))
        else:
            xd = torch.as_tensor(x.copy()).to(net.device).contiguous()
            jobs.append(dict(net=net, obs=xd, logits=True, actions=True, step=0))
        refs.append(ref)
    res = wh.forward_many(jobs)
    assert len(res) == len(MANY)
    for (seed, rows), (acts, lg), ref in zip(MANY, res, refs):
        check(f"{variant} {precision} forward_many seed {seed} rows {rows}", lg, acts, ref)
    return len(res)


def run_walk(wh, variant):
    """One bf16 launch of 256 * CUs + 289 rows (inputs() tiled), so some persistent workgroups take a
    second task; the reference on the first 300, the last 600 and every 97th row."""
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows = 256 * cus + 289
    w, x300, _ = case(variant, SEED[variant], 300, "bf16")
    x = np.ascontiguousarray(np.resize(x300, (rows, x300.shape[1])))
    pick = np.unique(np.concatenate([np.arange(300), np.arange(rows - 600, rows), np.arange(0, rows, 97)]))
    ref = reference(w, x[pick], "bf16")
    net = make_net(wh, variant, SEED[variant], "bf16", "host")
    acts, lg = net(torch.as_tensor(x).to(net.device).contiguous(), logits=True)
    check(f"{variant} bf16 walk of {rows} rows", lg, acts, ref, pick=pick)
    return rows, len(pick)


if __name__ == "__main__":   # the WH_MLP_LEGACY child of tests/test_gpu_mlp_exact.py: Medium and Large on k_mlp
    import os
    import sys

    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [ROOT, os.path.join(ROOT, "rllib-warehouse_amd")]
    import warehouse
    import warehouse.policy  # noqa: F401

    assert os.environ.get("WH_MLP_LEGACY") == "1"
    done = [(v, run_entry_points(make_net(warehouse, v, SEED[v], "bf16", "host"), v, 300, "bf16")) for v in ("medium", "large")]
    print("LEGACY EXACT OK", done)
