"""numpy model of the policy network's action tail (emit_row in csrc/mlp_common.h) -- TEST
INFRASTRUCTURE ONLY.

Every action the device policy takes leaves one function: given the nine f32 logits z of a row it
writes either their argmax (explore = 0) or a Gumbel-max sample of Categorical(z) (explore = 1).
This file restates that contract; the same one is documented in include/warehouse_amd.h
(wh_mlp_forward), DESIGN.md §3.4 and the stream table of oracle/philox.py.

    explore = 0   action = the FIRST maximum of z (numpy / torch argmax)
    explore = 1   key  = (seed & 0xffffffff, seed >> 32)
                  ctr  = (row & 0xffffffff, row >> 32, step, (5 << 24) | b),  b = 0, 1, 2
                  w_o  = word o of the 12 words of the three blocks (block o // 4, lane o % 4;
                         words 9-11 are unused)
                  u_o  = (f32(w_o >> 8) + 0.5f) * 2^-24, IN FLOAT32: a number in (0, 1], since for
                         w_o >> 8 = 0xFFFFFF the f32 sum 16777215.5 rounds (a tie, to even) to 2^24
                         and u_o is exactly 1
                  v_o  = z_o - log(-log(u_o)),  +inf where u_o = 1
                  action = the FIRST maximum of v

The model takes u_o in numpy float32, exactly as the kernel computes it, and the two logarithms in
float64; the device takes them with its fast f32 logarithm, so the two may differ on rows whose two
largest v are closer than the logarithms' error.  gumbel_actions returns that margin so a comparison
can leave such rows out."""
from __future__ import annotations

import numpy as np

from .philox import MLP as PUR_MLP
from .philox import philox4x32_10

NUM_ACTIONS = 9


def argmax_first(logits):
    """The explore = 0 rule: per row the index of the first maximum."""
    return np.argmax(np.asarray(logits), axis=1)


def sampler_words(seed, step, rows):
    """[len(rows), 12] uint64: the three Philox blocks (purpose 5) of each absolute row index."""
    rows = np.asarray(rows, np.uint64)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    out = np.empty((rows.shape[0], 12), np.uint64)
    for b in range(3):
        blk = philox4x32_10(rows & np.uint64(0xFFFFFFFF), rows >> np.uint64(32), step & 0xFFFFFFFF,
                            (PUR_MLP << 24) | b, k0, k1)
        for lane in range(4):
            out[:, 4 * b + lane] = blk[lane]
    return out


def uniform_f32(words):
    """u of a 32-bit word, in float32 as the kernel writes it: (f32(w >> 8) + 0.5f) * 2^-24."""
    w24 = (np.asarray(words, np.uint64) >> np.uint64(8)).astype(np.float32)
    u = (w24 + np.float32(0.5)) * np.float32(2.0 ** -24)
    assert u.dtype == np.float32
    return u


def gumbel_actions(logits_f32, seed, step, row0=0):
    """The explore = 1 rule for logits [N, 9] f32 of rows row0 .. row0 + N - 1.

    Returns (actions [N] int64, margin [N] float64, u [N, 9] float32): the first maximum of v, the
    difference of the two largest v (inf where one u is 1; nan -- compares false -- where two are)
    and the uniforms."""
    z = np.asarray(logits_f32)
    assert z.dtype == np.float32 and z.ndim == 2 and z.shape[1] == NUM_ACTIONS
    rows = np.arange(z.shape[0], dtype=np.uint64) + np.uint64(row0)
    u = uniform_f32(sampler_words(seed, step, rows)[:, :NUM_ACTIONS])
    with np.errstate(divide="ignore", invalid="ignore"):
        v = z.astype(np.float64) - np.log(-np.log(u.astype(np.float64)))
        top = np.sort(v, axis=1)
        margin = top[:, -1] - top[:, -2]
    return np.argmax(v, axis=1), margin, u
