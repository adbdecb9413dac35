"""Cases for the MLP training kernels (wh_mlp_train_forward / wh_mlp_backward, csrc/mlp_train.h): the
upstream gradients, a float64 reference of the backward pass, and a derived error bound.  Shared by
tests/test_mlp_grad_cpu.py (the conditions, without a GPU) and tests/test_gpu_mlp_grad.py.

Two kinds of case:
  * the integer-valued networks and inputs of tests/mlp_exact_cases.py with integer dlogits (dz): every
    product and partial sum of the forward AND the backward is exact in f32 (test_mlp_grad_cpu.py holds
    the condition), so the kernels must equal the float64 reference with tolerance 0;
  * a real-valued network (real_case): there the kernels may differ from float64 by rounding, at most
    by error_bound, which holds for ANY summation order and takes no measured constant.

Names follow include/warehouse_amd.h: h0 / h1 are the two hidden activations (mlp_exact_cases.reference
calls them h1 / h2, its h0 being x)."""
import numpy as np

import mlp_exact_cases as mc

KEYS = mc.KEYS
U = 2.0 ** -24                                  # unit roundoff of f32
ROWS_EXACT = (1, 31, 33, 257, 300)              # every variant; medium also at 513 (a third 256-row block, two K slices)
# ... and Small on both sides of the row count at which the kernels change their tile geometry (1,024 rows:
# the 32 x 32 tile, two K slices; 1,025: the 64 x 64 tile, three)
EXACT_CASES = tuple((v, r) for v in mc.VARIANTS for r in ROWS_EXACT) + (("medium", 513), ("small", 1024), ("small", 1025))
ROWS_REAL = (33, 513)


def dz(variant, rows):
    """[rows, 9] float32 integers in [-2, 2]; every fifth row (4, 9, ...) all zero."""
    rng = np.random.default_rng([41, mc.VARIANTS.index(variant), rows])
    d = rng.integers(-2, 3, (rows, 9)).astype(np.float32)
    d[4::5] = 0
    return d


def forward64(w, x):
    """The network in float64: pre0, h0, pre1, h1, logits."""
    f = np.float64
    W = {k: np.asarray(v, f) for k, v in w.items()}
    pre0 = np.asarray(x, f) @ W["w0"].T + W["b0"]
    h0 = np.maximum(pre0, 0)
    pre1 = h0 @ W["w1"].T + W["b1"]
    h1 = np.maximum(pre1, 0)
    return dict(pre0=pre0, h0=h0, pre1=pre1, h1=h1, logits=h1 @ W["w2"].T + W["b2"])


def reference_backward(w, x, dz, masks=None, fwd=None):
    """The six gradients in float64 (plus dh1, dh0 and the masks used).  masks = (m0, m1): the boolean
    h0 > 0 / h1 > 0 to use instead of the float64 forward's own."""
    f = np.float64
    fwd = fwd or forward64(w, x)
    m0, m1 = masks if masks is not None else (fwd["h0"] > 0, fwd["h1"] > 0)
    W = {k: np.asarray(v, f) for k, v in w.items()}
    d = np.asarray(dz, f)
    x = np.asarray(x, f)
    dh1 = (d @ W["w2"]) * m1
    dh0 = (dh1 @ W["w1"]) * m0
    return dict(w2=d.T @ fwd["h1"], b2=d.sum(0), w1=dh1.T @ fwd["h0"], b1=dh1.sum(0), w0=dh0.T @ x, b0=dh0.sum(0),
                dh1=dh1, dh0=dh0, masks=(m0, m1))


def forward_bound(w, x, fwd=None):
    """E(h0), E(h1), E(z): first-order running-error bounds of an f32 evaluation in any order."""
    fwd = fwd or forward64(w, x)
    A = {k: np.abs(np.asarray(v, np.float64)) for k, v in w.items()}
    in_dim, H0, H1 = A["w0"].shape[1], A["w0"].shape[0], A["w1"].shape[0]
    ax = np.abs(np.asarray(x, np.float64))
    e0 = (in_dim + 1) * U * (ax @ A["w0"].T + A["b0"])
    e1 = (H0 + 1) * U * (np.abs(fwd["h0"]) @ A["w1"].T + A["b1"]) + e0 @ A["w1"].T
    ez = (H1 + 1) * U * (np.abs(fwd["h1"]) @ A["w2"].T + A["b2"]) + e1 @ A["w2"].T
    return dict(h0=e0, h1=e1, logits=ez)


def simple_band(w, x, fwd=None):
    """K u (sum |w||h| + |b|) per hidden unit: forward_bound without the error its inputs carry."""
    fwd = fwd or forward64(w, x)
    A = {k: np.abs(np.asarray(v, np.float64)) for k, v in w.items()}
    in_dim, H0 = A["w0"].shape[1], A["w0"].shape[0]
    return dict(h0=(in_dim + 1) * U * (np.abs(np.asarray(x, np.float64)) @ A["w0"].T + A["b0"]),
                h1=(H0 + 1) * U * (np.abs(fwd["h0"]) @ A["w1"].T + A["b1"]))


def error_bound(w, x, dz, masks=None, fwd=None):
    """Per element, how far an f32 evaluation (fma chains in any order, u = 2^-24 per operation, first
    order) may lie from the float64 reference that uses the same masks: h0, h1, logits, w0 .. b2.
      E(dH1) = 9 u |dZ||W2|                  E(gW2) = rows u |dZ|^T |h1| + |dZ|^T E(h1)
      E(dH0) = H1 u |dH1||W1| + E(dH1)|W1|   E(gW1) = rows u |dH1|^T |h0| + E(dH1)^T |h0| + |dH1|^T E(h0)
                                             E(gW0) = rows u |dH0|^T |x| + E(dH0)^T |x|
    with |dH1|, |dH0| the reference's own values under the masks, E(dH) zero where the mask is, and the
    bias gradients with the second factor replaced by ones."""
    fwd = fwd or forward64(w, x)
    m0, m1 = masks if masks is not None else (fwd["h0"] > 0, fwd["h1"] > 0)
    A = {k: np.abs(np.asarray(v, np.float64)) for k, v in w.items()}
    H1 = A["w1"].shape[0]
    ax, ad = np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(dz, np.float64))
    rows = ax.shape[0]
    E = forward_bound(w, x, fwd)
    h0, h1 = np.abs(fwd["h0"]), np.abs(fwd["h1"])
    ref = reference_backward(w, x, dz, masks=(m0, m1), fwd=fwd)
    a1, a0 = np.abs(ref["dh1"]), np.abs(ref["dh0"])      # |dH1|, |dH0| of the reference under these masks
    e_dh1 = 9 * U * (ad @ A["w2"]) * m1
    e_dh0 = (H1 * U * (a1 @ A["w1"]) + e_dh1 @ A["w1"]) * m0
    E["w2"] = rows * U * (ad.T @ h1) + ad.T @ E["h1"]
    E["b2"] = rows * U * ad.sum(0)
    E["w1"] = rows * U * (a1.T @ h0) + e_dh1.T @ h0 + a1.T @ E["h0"]
    E["b1"] = rows * U * a1.sum(0) + e_dh1.sum(0)
    E["w0"] = rows * U * (a0.T @ ax) + e_dh0.T @ ax
    E["b0"] = rows * U * a0.sum(0) + e_dh0.sum(0)
    return E


def backward_worst(w, x, dz, fwd=None):
    """Per backward product, the largest sum |a||b| of any of its dot products, in grains of 2^-2 (one
    input row holds quarters, and a weight gradient sums over all rows)."""
    fwd = fwd or forward64(w, x)
    A = {k: np.abs(np.asarray(v, np.float64)) for k, v in w.items()}
    ref = reference_backward(w, x, dz, fwd=fwd)
    ad, ax = np.abs(np.asarray(dz, np.float64)), np.abs(np.asarray(x, np.float64))
    dh1, dh0 = np.abs(ref["dh1"]), np.abs(ref["dh0"])
    sums = dict(dh1=ad @ A["w2"], w2=ad.T @ np.abs(fwd["h1"]), b2=ad.sum(0), dh0=dh1 @ A["w1"],
                w1=dh1.T @ np.abs(fwd["h0"]), b1=dh1.sum(0), w0=dh0.T @ ax, b0=dh0.sum(0))
    return {k: float(v.max()) * 4 for k, v in sums.items()}


def shuffled_backward_f32(w, x, dz, seed):
    """The backward in float32, every product accumulated one k at a time in a shuffled order: under the
    exactness condition the order cannot matter.  The masks are the float32 forward's own h > 0."""
    rng = np.random.default_rng(seed)
    f = np.float32

    def matmul(a, b):                      # a [M, K] @ b [K, N], k shuffled
        acc = np.zeros((a.shape[0], b.shape[1]), f)
        for k in rng.permutation(a.shape[1]):
            acc += a[:, k:k + 1] * b[k:k + 1, :]
        return acc

    x, d = np.asarray(x, f), np.asarray(dz, f)
    h0 = np.maximum(matmul(x, w["w0"].T) + w["b0"], f(0))
    h1 = np.maximum(matmul(h0, w["w1"].T) + w["b1"], f(0))
    ones = np.ones((x.shape[0], 1), f)
    dh1 = matmul(d, w["w2"]) * (h1 > 0)
    dh0 = matmul(dh1, w["w1"]) * (h0 > 0)
    return dict(w2=matmul(d.T, h1), b2=matmul(d.T, ones)[:, 0], w1=matmul(dh1.T, h0), b1=matmul(dh1.T, ones)[:, 0],
                w0=matmul(dh0.T, x), b0=matmul(dh0.T, ones)[:, 0], h0=h0, h1=h1)


def swap_rows(w, key, i=3, j=7):
    """w with rows i and j of matrix `key` exchanged (its bias stays): a misplaced-weight mutant."""
    m = dict(w)
    a = w[key].copy()
    a[[i, j]] = a[[j, i]]
    m[key] = a
    return m


# ----------------------------------------------------------------------------- the cases, computed once
_exact, _real = {}, {}


def exact_case(variant, rows):
    """(w, x, dz, forward, backward) of an integer-valued case: float64, shared, never written."""
    key = (variant, rows)
    if key not in _exact:
        w, x = mc.network(variant, mc.SEED[variant]), mc.inputs(variant, mc.SEED[variant], rows)
        d = dz(variant, rows)
        fwd = forward64(w, x)
        for a in list(w.values()) + [x, d]:
            a.setflags(write=False)
        _exact[key] = (w, x, d, fwd, reference_backward(w, x, d, fwd=fwd))
    return _exact[key]


def real_case(variant, rows):
    """(w, x, dz, forward) of the real-valued case: nn.Linear-style uniform weights (seed 3), x uniform
    in [-1, 1]."""
    from warehouse.policy import init_weights

    key = (variant, rows)
    if key not in _real:
        w = init_weights(*mc.VARIANT_DIMS[variant], seed=3)
        x = np.random.default_rng([5, rows]).uniform(-1, 1, (rows, mc.VARIANT_DIMS[variant][0])).astype(np.float32)
        d = dz(variant, rows)
        for a in list(w.values()) + [x, d]:
            a.setflags(write=False)
        _real[key] = (w, x, d, forward64(w, x))
    return _real[key]


def in_band(fwd, E):
    """Per layer, the hidden units whose float64 pre-activation lies within the forward bound of 0: the
    only ones whose mask an f32 evaluation may decide differently."""
    return np.abs(fwd["pre0"]) <= E["h0"], np.abs(fwd["pre1"]) <= E["h1"]
