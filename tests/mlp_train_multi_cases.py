"""Cases for the multi-network training entry points (wh_mlp_train_forward_multi /
wh_mlp_backward_multi, csrc/mlp_train.h): up to four integer-valued networks of one shape and one row
count, each with its float64 reference.  Shared by tests/test_mlp_train_multi_cpu.py (the condition that
gives tolerance 0 its meaning, without a GPU) and tests/test_gpu_mlp_train_multi.py.

Job k < 3 is the integer network mlp_exact_cases.network(variant, s) on mlp_exact_cases.inputs(variant, s,
rows) with s = SEEDS[k] and the integer dz of dz() below; job 3 is mlp_grad_cases.exact_case(variant,
rows) itself.  The three seeds give three different networks, inputs and gradients, so a launch that
hands a workgroup the pointers of the wrong network cannot pass.

SHAPES are the smallest that reach: a single row; the 32-row tile edge; a ragged tail; two K slices plus
the reduce launch on the Deep geometry; the Wide geometry with three slices; the 145-wide and
1,024-wide edges.  (small, 1025) is the tightest against the exactness limit (1.52e7 of 2^24): it takes
no more rows."""
import numpy as np

import mlp_exact_cases as mc
import mlp_grad_cases as mg

KEYS = mc.KEYS
SEEDS = (21, 22, 23)
SHAPES = (("small", 1), ("small", 33), ("small", 300), ("medium", 513), ("small", 1025), ("large", 33))
# the bit-equality runs on real-valued weights: (variant, rows), and the init_weights seeds of the jobs
REAL_SHAPES = (("medium", 257), ("medium", 513), ("large", 513), ("small", 1025))
REAL_SEEDS = (3, 4, 5, 6)


def dz(seed, rows):
    """[rows, 9] float32 integers in [-2, 2]."""
    return np.random.default_rng([41, seed, rows]).integers(-2, 3, (rows, 9)).astype(np.float32)


_jobs = {}


def job(variant, rows, k):
    """(w, x, dz, forward, backward) of job k of a shape: float64 references, shared, never written."""
    if k == 3:
        return mg.exact_case(variant, rows)
    key = (variant, rows, k)
    if key not in _jobs:
        s = SEEDS[k]
        w, x, d = mc.network(variant, s), mc.inputs(variant, s, rows), dz(s, rows)
        fwd = mg.forward64(w, x)
        for a in list(w.values()) + [x, d]:
            a.setflags(write=False)
        _jobs[key] = (w, x, d, fwd, mg.reference_backward(w, x, d, fwd=fwd))
    return _jobs[key]


_real = {}


def real_job(variant, rows, k):
    """(w, x, dz) of job k of a real-valued run: init_weights(seed REAL_SEEDS[k]), x uniform in [-1, 1].
    Jobs 0 and 1 share one x (the test gives them one device pointer)."""
    from warehouse.policy import init_weights

    key = (variant, rows, k)
    if key not in _real:
        w = init_weights(*mc.VARIANT_DIMS[variant], seed=REAL_SEEDS[k])
        x = np.random.default_rng([5, rows, max(k, 1)]).uniform(-1, 1, (rows, mc.VARIANT_DIMS[variant][0])).astype(np.float32)
        d = np.random.default_rng([7, rows, k]).uniform(-1, 1, (rows, 9)).astype(np.float32)
        for a in list(w.values()) + [x, d]:
            a.setflags(write=False)
        _real[key] = (w, x, d)
    return _real[key]
