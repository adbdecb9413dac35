"""Test bodies of the replay priority tree (wh_replay_prio_*, csrc/prio.h; ReplayBuffer(prioritized=True)).

tests/test_gpu_prio.py runs them on the GPU, tests/test_prio_cpu.py on the host engine.  Tree-level
bodies take `(lib, device)` and go through the C ABI with sentinel guards behind every buffer;
buffer-level bodies take an env factory like tests/replay_cases.py.  The numpy model of the tree is
here: quantisation, level sums recomputed from the leaves, the inverse CDF as np.cumsum on uint64 +
searchsorted, the philox masses from oracle/philox.py with Python integers for the 64 x 64 high
product.  Every comparison is at tolerance 0 except the importance weights.

The small counts (COUNTS, one to four levels) take the full sequences; so do DEEP_COUNTS (five and
six levels, the sizes a real buffer has).  Seven levels take a reduced sequence with few whole-tree
copies, eight levels a tree that is almost all zeros against SparseModel; case_launch_widths and
case_unaligned_fills are the launches of thousands of workgroups.
"""
import ctypes

import numpy as np
import torch

from oracle import philox as oph

ONE, QMAX = 1 << 20, 0x7FFFFFFF
COUNTS = (1, 16, 17, 333, 4099)          # 1, 1, 2, 3, 4 levels above the leaves
# 65,537: five levels, the last leaf alone in its entry at every level; 2^20: five levels and no
# padding anywhere; 2^20 + 1: six levels
DEEP_COUNTS = (65537, 1 << 20, (1 << 20) + 1)
COUNT_7, COUNT_8 = (1 << 24) + 1, (1 << 28) + 1   # seven levels (reduced body), eight (sparse body)


def levels_of(count):
    """Levels above the leaves: the smallest K >= 1 with 16^K >= count."""
    k = 1
    while 16 ** k < count:
        k += 1
    return k


LEVELS = {c: levels_of(c) for c in COUNTS + DEEP_COUNTS + (COUNT_7, COUNT_8)}
GUARD = 256
SEED = 0x5EED0000BEEF
MASK64 = (1 << 64) - 1


# ----------------------------------------------------------------------------- the model
def shape(count):
    """(leaf_words, node_words, [(n_k, off_k) for k = 1 ..]) of a tree of `count` leaves."""
    pad = lambda n: (n + 15) // 16 * 16   # noqa: E731
    levels, n, off = [], count, 0
    while True:
        n = (n + 15) // 16
        levels.append((n, off))
        off += pad(n)
        if n == 1:
            return pad(count), off, levels


def quantise(p):
    """The header's rule on f32 values (NaN or x < 1 -> 1; x >= 2^31 -> 2^31 - 1; else truncate)."""
    p = np.asarray(p, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        x = p * np.float32(1048576.0)
        q = np.ones(p.shape, np.uint32)
        mid = (x >= 1) & (x < 2147483648.0)
        q[mid] = x[mid].astype(np.uint32)
        q[x >= 2147483648.0] = QMAX
    return q


class Model:
    def __init__(self, count):
        self.count = count
        self.leaf = np.zeros(count, np.uint32)
        self.max_q = ONE

    def fill(self, first, n, mode, q=0):
        self.leaf[first:first + n] = self.max_q if mode else q

    def update(self, idx, p):
        idx, q = np.asarray(idx, np.int64), quantise(p)
        ok = (idx >= 0) & (idx < self.count)
        idx, q = idx[ok], q[ok]
        self.leaf[idx] = 0
        np.maximum.at(self.leaf, idx, q)                      # duplicates: the largest q wins
        if len(q):
            self.max_q = max(self.max_q, int(q.max()))

    def arrays(self):
        """leaf [leaf_words] and node [node_words], every sum recomputed from the leaves."""
        lw, nw, levels = shape(self.count)
        leaf = np.zeros(lw, np.uint32)
        leaf[:self.count] = self.leaf
        node, cur = np.zeros(nw, np.uint64), leaf.astype(np.uint64)
        for n, off in levels:
            sums = cur.reshape(-1, 16).sum(axis=1, dtype=np.uint64)
            assert len(sums) == n
            node[off:off + n] = sums
            cur = node[off:off + (n + 15) // 16 * 16]
        return leaf, node

    def total(self):
        return int(self.leaf.astype(np.uint64).sum(dtype=np.uint64))

    def sample(self, r):
        """(idx, q) for the 64-bit draws r (Python ints): mass = r * total >> 64, then the first
        leaf whose inclusive prefix sum exceeds it."""
        total = self.total()
        if total == 0:
            return np.full(len(r), -1, np.int64), np.zeros(len(r), np.uint32)
        c = np.cumsum(self.leaf.astype(np.uint64), dtype=np.uint64)
        mass = np.array([(int(x) * total) >> 64 for x in r], np.uint64)
        idx = np.searchsorted(c, mass, side="right").astype(np.int64)
        return idx, self.leaf[idx]


class SparseModel:
    """Model for trees too large for a dense host copy: the non-zero leaves as a sorted index array
    and their values.  tests/test_prio_cpu.py holds it equal to Model on the same operations."""

    def __init__(self, count):
        self.count = count
        self.idx = np.zeros(0, np.int64)
        self.val = np.zeros(0, np.uint32)
        self.max_q = ONE

    def _replace(self, idx, val):
        """Leaves `idx` (unique) take `val`; a zero value removes the leaf."""
        keep = ~np.isin(self.idx, idx)
        idx, val = idx[val > 0], val[val > 0]
        ai, av = np.concatenate([self.idx[keep], idx]), np.concatenate([self.val[keep], val])
        order = np.argsort(ai, kind="stable")
        self.idx, self.val = ai[order], av[order].astype(np.uint32)

    def fill(self, first, n, mode, q=0):
        self._replace(np.arange(first, first + n, dtype=np.int64), np.full(n, self.max_q if mode else q, np.uint32))

    def update(self, idx, p):
        idx, q = np.asarray(idx, np.int64), quantise(p)
        ok = (idx >= 0) & (idx < self.count)
        idx, q = idx[ok], q[ok]
        if not len(q):
            return
        order = np.lexsort((q, idx))                                  # by leaf, then by q: a leaf's last is its largest
        idx, q = idx[order], q[order]
        last = np.append(idx[1:] != idx[:-1], True)
        self._replace(idx[last], q[last])
        self.max_q = max(self.max_q, int(q.max()))

    def level(self, k):
        """(indices, values as uint64) of the non-zero entries of level k (0: the leaves)."""
        if k == 0:
            return self.idx, self.val.astype(np.uint64)
        u, inv = np.unique(self.idx >> (4 * k), return_inverse=True)
        s = np.zeros(len(u), np.uint64)
        np.add.at(s, inv, self.val.astype(np.uint64))
        return u, s

    def total(self):
        return int(self.val.astype(np.uint64).sum(dtype=np.uint64))

    def sample(self, r):
        total = self.total()
        if total == 0:
            return np.full(len(r), -1, np.int64), np.zeros(len(r), np.uint32)
        c = np.cumsum(self.val.astype(np.uint64), dtype=np.uint64)
        mass = np.array([(int(x) * total) >> 64 for x in r], np.uint64)
        at = np.searchsorted(c, mass, side="right")
        return self.idx[at], self.val[at]


def philox_draws(seed, draw, M):
    m = np.arange(M, dtype=np.uint64)
    c = oph.philox4x32_10(m, draw & 0xFFFFFFFF, draw >> 32, 7 << 24, seed & 0xFFFFFFFF, seed >> 32)
    return [(int(a) << 32) | int(b) for a, b in zip(c[0], c[1])]


def draw_for_mass(mass, total):
    """The smallest r with (r * total) >> 64 == mass."""
    r = -((-mass << 64) // total)
    assert r <= MASK64 and (r * total) >> 64 == mass
    return r


# ----------------------------------------------------------------------------- a tree behind the C ABI
def _guarded(nbytes, device, fill=0):
    # (zeros, not a fill: an eight-level tree's 1.1 GB of leaves are never touched on the host)
    raw = torch.full((nbytes + GUARD,), fill, dtype=torch.uint8, device=device) if fill else \
        torch.zeros(nbytes + GUARD, dtype=torch.uint8, device=device)
    raw[nbytes:] = 0xA5
    return raw


class Tree:
    """Buffers of exactly the queried sizes, each followed by GUARD sentinel bytes, and the entry
    points of one library on them."""

    def __init__(self, nat, lib, device, count):
        self.nat, self.lib, self.device, self.count = nat, lib, device, count
        lw, nw, lv = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
        assert lib.wh_replay_prio_query(count, ctypes.byref(lw), ctypes.byref(nw), ctypes.byref(lv)) == nat.WH_OK
        assert (lw.value, nw.value, lv.value) == (shape(count)[0], shape(count)[1], len(shape(count)[2]))
        self.sizes = dict(leaf=4 * lw.value, node=8 * nw.value, max_q=4)
        self.raw = {k: _guarded(n, device) for k, n in self.sizes.items()}
        self.raw["max_q"][:4] = torch.tensor(list(ONE.to_bytes(4, "little")), dtype=torch.uint8)
        self.keep = []

    def struct(self):
        return self.nat.WhReplayPrio(self.raw["leaf"].data_ptr(), self.raw["node"].data_ptr(),
                                     self.raw["max_q"].data_ptr(), self.count)

    def _stream(self):
        return self.nat.stream_of(torch.device(self.device))

    def fill(self, first, n, mode, q=0):
        rc = self.lib.wh_replay_prio_fill(ctypes.byref(self.struct()), first, n, mode, q, self._stream())
        assert rc == self.nat.WH_OK, rc

    def update(self, idx, p):
        ix = torch.as_tensor(np.ascontiguousarray(idx, np.int64)).to(self.device)
        pp = torch.as_tensor(np.ascontiguousarray(p, np.float32)).to(self.device)
        rc = self.lib.wh_replay_prio_update(ctypes.byref(self.struct()), len(ix), ix.data_ptr(), pp.data_ptr(),
                                            self._stream())
        assert rc == self.nat.WH_OK, rc

    def sample(self, M, u=None, seed=SEED, draw=0):
        """(idx, q, total) as numpy, the outputs guarded."""
        out = dict(idx=_guarded(8 * M, self.device, 0x5A), q=_guarded(4 * M, self.device, 0x5A),
                   total=_guarded(8, self.device, 0x5A))
        up = None
        if u is not None:
            ut = torch.as_tensor(np.array([int(x) for x in u], np.uint64).view(np.int64)).to(self.device)
            up = ut.data_ptr()
        rc = self.lib.wh_replay_prio_sample(ctypes.byref(self.struct()), M, up, seed, draw, out["idx"].data_ptr(),
                                            out["q"].data_ptr(), out["total"].data_ptr(), self._stream())
        assert rc == self.nat.WH_OK, rc
        host = {k: v.cpu().numpy() for k, v in out.items()}
        for k, v in host.items():
            assert (v[-GUARD:] == 0xA5).all(), f"bytes written past the end of {k}_out"
        return (host["idx"][:8 * M].view(np.int64), host["q"][:4 * M].view(np.uint32),
                int(host["total"][:8].view(np.uint64)[0]))

    def read(self):
        """(leaf, node, max_q) as numpy; the guards checked."""
        host = {k: v.cpu().numpy() for k, v in self.raw.items()}
        for k, v in host.items():
            assert (v[-GUARD:] == 0xA5).all(), f"bytes written past the end of {k}"
        return (host["leaf"][:self.sizes["leaf"]].view(np.uint32), host["node"][:self.sizes["node"]].view(np.uint64),
                int(host["max_q"][:4].view(np.uint32)[0]))

    def check(self, model, what=""):
        """Every node the sum of its children, all padding zero, the root the sum of the leaves,
        max_q the model's: the buffers equal the model's arrays."""
        leaf, node, max_q = self.read()
        want_leaf, want_node = model.arrays()
        np.testing.assert_array_equal(leaf, want_leaf, err_msg=f"{what}: leaves")
        np.testing.assert_array_equal(node, want_node, err_msg=f"{what}: sums")
        assert not leaf[self.count:].any() and int(node[shape(self.count)[2][-1][1]]) == model.total(), what
        assert max_q == model.max_q, f"{what}: max_q {max_q}, expected {model.max_q}"

    def leaf_at(self, idx):
        """leaf[idx] as numpy uint32, indexed on the buffer's own device (no whole-tree copy)."""
        leaf = self.raw["leaf"][:self.sizes["leaf"]].view(torch.int32)
        return leaf[torch.as_tensor(np.asarray(idx, np.int64)).to(self.device)].cpu().numpy().view(np.uint32)

    def check_sparse(self, model, what=""):
        """check() against a SparseModel without a dense host copy: per level, the non-zero entries
        of the level's whole slice (padding included) by torch.nonzero on the buffer's device, their
        indices and values the model's; the guards and max_q read on their own."""
        lw, nw, levels = shape(self.count)
        leaf = self.raw["leaf"][:self.sizes["leaf"]].view(torch.int32)
        node = self.raw["node"][:self.sizes["node"]].view(torch.int64)
        assert len(levels) == LEVELS[self.count]
        for k in range(len(levels) + 1):
            if k == 0:
                part = leaf
            else:
                n, off = levels[k - 1]
                part = node[off:off + (n + 15) // 16 * 16]
            at = torch.nonzero(part).flatten()
            got_idx, got_val = at.cpu().numpy(), part[at].cpu().numpy()
            got_val = got_val.view(np.uint32).astype(np.uint64) if k == 0 else got_val.view(np.uint64)
            want_idx, want_val = model.level(k)
            np.testing.assert_array_equal(got_idx, want_idx, err_msg=f"{what}: level {k}, non-zero entries")
            np.testing.assert_array_equal(got_val, want_val, err_msg=f"{what}: level {k}, values")
        root = levels[-1][1]
        assert int(node[root].item()) == model.total(), what
        for k, v in self.raw.items():
            assert bool((v[self.sizes[k]:] == 0xA5).all()), f"bytes written past the end of {k}"
        max_q = int(self.raw["max_q"][:4].cpu().numpy().view(np.uint32)[0])
        assert max_q == model.max_q, f"{what}: max_q {max_q}, expected {model.max_q}"

    def free(self):
        """Drop the buffers (and hand a device's cached blocks back) before the next test."""
        self.raw = {}
        if str(self.device) != "cpu":
            torch.cuda.empty_cache()


QUANT_TABLE = np.array([np.nan, 0.0, -0.0, -3.5, 1e-9, 2.0 ** -20, 1.0, 2047.9, 2048.0, 1e30, np.inf], np.float32)
# 2047.9 as f32 is a multiple of 2^-13, so times 2^20 it is a whole number, exact in float64 too
Q_2047_9 = int(float(np.float32(2047.9)) * 1048576.0)
QUANT_WANT = np.array([1, 1, 1, 1, 1, 1, ONE, Q_2047_9, QMAX, QMAX, QMAX], np.uint32)


def case_quantisation_model():
    """The model's quantisation gives the header's table, worked out without it."""
    np.testing.assert_array_equal(quantise(QUANT_TABLE), QUANT_WANT)
    assert float(np.float32(2047.9)) * 8192 == 16776397 and Q_2047_9 == 16776397 * 128 and Q_2047_9 < QMAX


# ----------------------------------------------------------------------------- 1. fills and updates
def case_tree_ops(nat, lib, device, count):
    """A sequence of fills and updates, the whole tree checked against the model after each.  Returns
    the final (leaf, node, max_q), which the GPU suite compares between the engines."""
    t, m = Tree(nat, lib, device, count), Model(count)
    assert len(shape(count)[2]) == LEVELS[count]
    rng = np.random.default_rng(count)
    t.check(m, "empty")

    def both(op, *args):
        getattr(t, op)(*args)
        getattr(m, op)(*args)
        t.check(m, f"count {count}: {op}{args[:3] if op == 'fill' else (len(args[0]),)}")

    both("fill", 0, count, 0, ONE)                                    # the whole tree
    first = min(5, count - 1)
    both("fill", first, min(count - first, 20), 0, 3)                 # starts and ends mid-node
    both("fill", count - 1, 1, 0, 12345)                              # a range of 1
    both("fill", count // 2, 1, 0, QMAX)
    both("fill", 0, 0, 0, 7)                                          # n = 0: nothing
    # the quantisation table, spread over the tree (count < 11: duplicates, the largest q wins)
    idx = (np.arange(len(QUANT_TABLE)) * 389) % count
    both("update", idx, QUANT_TABLE)
    if count >= 4099:
        np.testing.assert_array_equal(t.read()[0][idx], QUANT_WANT)
    assert m.max_q == QMAX
    t2, m2 = Tree(nat, lib, device, count), Model(count)              # max_q raised by an update, then mode 1
    for tt in (t2, m2):
        tt.update([count - 1], [3.25])
        tt.fill(0, max(1, count // 3), 1)
    t2.check(m2, "mode 1")
    assert m2.max_q == 3407872 and (t2.read()[0][:max(1, count // 3)] == 3407872).all()
    for M in (1, 255, 256, 257, 1000):
        idx = rng.integers(0, count, M)
        p = rng.uniform(0.0, 40.0, M).astype(np.float32)
        if M > 2:
            idx[1] = idx[2]                                           # duplicates within a workgroup
            idx[M // 2] = -1                                          # ignored
        if M > 256:
            idx[-1] = idx[0]                                          # ... and across workgroups
            idx[7], idx[300 % M] = count, 1 << 40                     # ignored
        both("update", idx, p)
    both("update", np.array([-1, count, 1 << 40]), np.array([5.0, 6.0, 7.0], np.float32))   # nothing valid
    both("fill", count // 4, max(1, count // 2), 0, 0)                # q = 0 clears
    both("fill", 0, count, 1)                                         # mode 1 over the whole tree
    both("fill", 0, count, 0, 0)
    assert m.total() == 0
    both("update", rng.integers(0, count, 300), rng.uniform(0.0, 2.0, 300).astype(np.float32))
    return t.read()


# ----------------------------------------------------------------------------- 2. sampling
def sparse_tree(nat, lib, device, count, seed):
    """Positive leaves with long zero runs between them (and zero runs at both ends for large counts)."""
    t, m = Tree(nat, lib, device, count), Model(count)
    rng = np.random.default_rng(seed)
    if count <= 17:
        idx = np.arange(count)[::3]
    else:
        idx = np.unique(np.concatenate([rng.integers(count // 8, count // 4, 9), rng.integers(count // 2, count - 3, 30),
                                        [count - 4]]))
    p = rng.uniform(1e-4, 30.0, len(idx)).astype(np.float32)
    for tt in (t, m):
        tt.update(idx, p)
    t.check(m, "sparse")
    return t, m


def assert_samples(t, m, M, u=None, draw=0, what=""):
    idx, q, total = t.sample(M, u=u, draw=draw)
    r = philox_draws(SEED, draw, M) if u is None else u
    want_idx, want_q = m.sample(r)
    np.testing.assert_array_equal(idx, want_idx, err_msg=f"{what} M={M}: idx")
    np.testing.assert_array_equal(q, want_q, err_msg=f"{what} M={M}: q")
    assert total == m.total(), what
    if total:
        # q_out == leaf[idx_out] (from seven levels up read at idx alone, not through a whole-tree copy)
        np.testing.assert_array_equal(q, t.read()[0][idx] if t.count <= DEEP_COUNTS[-1] else t.leaf_at(idx))
        assert (q > 0).all()
    return idx


def case_sampling(nat, lib, device, count):
    """Philox and injected draws against the model's inverse CDF, for every row / wave / workgroup
    split of M; the ends and the prefix boundaries of the CDF; large sums; the empty tree."""
    rng = np.random.default_rng(100 + count)
    t, m = sparse_tree(nat, lib, device, count, 3)
    pos = np.flatnonzero(m.leaf)
    total = m.total()
    for M in (1, 15, 16, 17, 63, 65, 1000):
        assert_samples(t, m, M, draw=(5 << 32) | M, what=f"count {count} philox")
        u = [int(x) for x in rng.integers(0, 1 << 64, M, dtype=np.uint64)]
        assert_samples(t, m, M, u=u, what=f"count {count} injected")
    ends = assert_samples(t, m, 2, u=[0, MASK64], what="ends")
    assert ends[0] == pos[0] and ends[1] == pos[-1]
    # on every prefix boundary and one below it: mass == c[i] starts the next positive leaf
    c = np.cumsum(m.leaf.astype(np.uint64), dtype=np.uint64)
    u, want = [], []
    for a, b in zip(pos[:-1], pos[1:]):
        u += [draw_for_mass(int(c[a]) - 1, total), draw_for_mass(int(c[a]), total)]
        want += [a, b]
    if u:
        got = assert_samples(t, m, len(u), u=u, what="boundaries")
        np.testing.assert_array_equal(got, want)
    # one leaf at 2^31 - 1 among ones
    t, m = Tree(nat, lib, device, count), Model(count)
    for tt in (t, m):
        tt.fill(0, count, 0, 1)
        tt.fill(count * 2 // 3, 1, 0, QMAX)
    got = assert_samples(t, m, 65, draw=9, what="one big leaf")
    assert count == 1 or (got == count * 2 // 3).sum() >= 60
    assert_samples(t, m, 3, u=[0, draw_for_mass(m.total() - 1, m.total()), MASK64], what="one big leaf, ends")
    # every leaf at 2^31 - 1: the largest sums a tree of this size holds
    for tt in (t, m):
        tt.fill(0, count, 0, QMAX)
    t.check(m, "all max")
    assert m.total() == count * QMAX
    got = assert_samples(t, m, 1000, draw=11, what="all max")
    assert count < 333 or len(np.unique(got)) > 200
    assert_samples(t, m, 2, u=[0, MASK64], what="all max, ends")
    # the empty tree
    for tt in (t, m):
        tt.fill(0, count, 0, 0)
    idx, q, total = t.sample(17, draw=1)
    assert (idx == -1).all() and not q.any() and total == 0
    idx, q, total = t.sample(3, u=[0, 5, MASK64])
    assert (idx == -1).all() and not q.any() and total == 0


# ----------------------------------------------------------------------------- 3. between the engines
def case_portability(nat, count):
    """The same operations on the device and on the host engine leave byte-identical trees, and the
    device's tree copied to host memory samples the same indices there."""
    dev = case_tree_ops(nat, nat.lib(), "cuda:0", count)
    host = case_tree_ops(nat, nat.host_lib(), "cpu", count)
    for a, b, what in zip(dev, host, ("leaf", "node", "max_q")):
        np.testing.assert_array_equal(a, b, err_msg=what)
    td, md = sparse_tree(nat, nat.lib(), "cuda:0", count, 8)
    th = Tree(nat, nat.host_lib(), "cpu", count)
    for k in th.raw:
        th.raw[k].copy_(td.raw[k].cpu())
    for M, draw in ((70, 3), (1000, 1 << 33)):
        a, b = td.sample(M, draw=draw), th.sample(M, draw=draw)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
        assert a[2] == b[2]
        np.testing.assert_array_equal(a[0], md.sample(philox_draws(SEED, draw, M))[0])


# ----------------------------------------------------------------------------- 4. seven and eight levels
def case_seven_levels(nat, lib, device):
    """16,777,217 leaves, seven levels: a reduced sequence (the full one would copy 73 MB back per
    operation), the whole tree compared with the model after each of its six steps."""
    count = COUNT_7
    assert len(shape(count)[2]) == LEVELS[count] == 7
    t, m = Tree(nat, lib, device, count), Model(count)
    rng = np.random.default_rng(7)
    try:
        def both(what, op, *args):
            getattr(t, op)(*args)
            getattr(m, op)(*args)
            t.check(m, f"seven levels: {what}")

        both("whole-tree fill", "fill", 0, count, 0, ONE)
        # off a workgroup's 256, over a level-5 entry boundary (a multiple of 2^20), 587 workgroups
        first, n = 5 * (1 << 20) - 70001, 150000
        assert first % 256 and (first >> 20) + 1 == (first + n - 1) >> 20
        both("unaligned fill", "fill", first, n, 0, int(rng.integers(1, QMAX)))
        M = 5000
        idx, p = rng.integers(0, count, M), rng.uniform(0.0, 40.0, M).astype(np.float32)
        idx[1], idx[M - 1] = idx[2], idx[0]                           # duplicates within and across workgroups
        idx[5], idx[6] = count - 1, first + 3
        idx[10], idx[300], idx[4000] = -1, count, 1 << 40             # ignored
        both("update", "update", idx, p)
        # philox and injected draws, the ends, and the prefix boundaries on both sides of that fill
        assert_samples(t, m, 4096, draw=(7 << 32) | 1, what="seven levels philox")
        u = [int(x) for x in rng.integers(0, 1 << 64, 1000, dtype=np.uint64)]
        assert_samples(t, m, len(u), u=u, what="seven levels injected")
        ends = assert_samples(t, m, 2, u=[0, MASK64], what="seven levels ends")
        assert list(ends) == [0, count - 1]
        c, total = np.cumsum(m.leaf.astype(np.uint64), dtype=np.uint64), m.total()
        assert m.leaf.all()
        u = [draw_for_mass(int(c[i]) - d, total) for i in (first - 1, first + n - 1) for d in (1, 0)]
        got = assert_samples(t, m, 4, u=u, what="seven levels boundaries")
        assert list(got) == [first - 1, first, first + n - 1, first + n]
        t.check(m, "seven levels: after the samples")
        both("all max", "fill", 0, count, 0, QMAX)
        assert m.total() == count * QMAX and m.total() > 1 << 54
        got = assert_samples(t, m, 1000, draw=11, what="seven levels all max")
        assert len(np.unique(got >> 20)) >= 16                        # under every full level-5 entry
        ends = assert_samples(t, m, 2, u=[0, MASK64], what="seven levels all max, ends")
        assert list(ends) == [0, count - 1]
        both("empty", "fill", 0, count, 0, 0)
        assert m.total() == 0
        for kw in (dict(draw=1), dict(u=[0, 5, MASK64])):
            idx, q, total = t.sample(3, **kw)
            assert (idx == -1).all() and not q.any() and total == 0
    finally:
        t.free()


def case_eight_levels_sparse(nat, lib, device):
    """2^28 + 1 leaves, eight levels (1.1 GB of leaves, all but some 70,000 zero) against SparseModel,
    every level checked by its non-zero entries on the buffer's own device.  The root of this tree
    has two children (leaves 0 .. 2^28 - 1 and the last leaf alone); level 6, with 17 entries of
    2^24 leaves each, is the highest level with more than two, so the spread of the philox sample
    is asserted over three of those."""
    count = COUNT_8
    assert len(shape(count)[2]) == LEVELS[count] == 8 and shape(count)[2][-2][0] == 2
    t, m = Tree(nat, lib, device, count), SparseModel(count)
    rng = np.random.default_rng(8)
    try:
        def both(what, op, *args):
            getattr(t, op)(*args)
            getattr(m, op)(*args)
            t.check_sparse(m, f"eight levels: {what}")

        t.check_sparse(m, "eight levels: empty")
        idx = rng.integers(1 << 20, count - (1 << 20), 300)
        both("random update", "update", idx, rng.uniform(1e-3, 30.0, 300).astype(np.float32))
        ends = assert_samples(t, m, 2, u=[0, MASK64], what="eight levels ends")
        assert list(ends) == [idx.min(), idx.max()]                   # the first and last non-zero leaf
        edge = np.array([0, 15, 16, (1 << 24) - 1, 1 << 24, (1 << 28) - 1, 1 << 28, -1, (1 << 31) + 5, 777777, 777777])
        p = rng.uniform(1e-3, 30.0, len(edge)).astype(np.float32)
        both("update at the edges", "update", edge, p)
        valid = edge[(edge >= 0) & (edge < count)]
        assert (t.leaf_at(valid) > 0).all() and t.leaf_at([777777])[0] == quantise(p[-2:]).max()
        # from an unaligned start over a level-6 entry boundary (a multiple of 2^24)
        first, n = 3 * (1 << 24) - 33001, 70000
        assert first % 256 and (first >> 24) + 1 == (first + n - 1) >> 24
        both("fill over a level-6 boundary", "fill", first, n, 0, int(rng.integers(1, ONE)))
        # the last 300 leaves at a q that gives them 1/17 of the total: about 240 of 4,096 rows
        q = m.total() // (16 * 300)
        assert 5 < q <= QMAX
        both("fill of the last 300", "fill", count - 300, 300, 0, q)
        got = assert_samples(t, m, 4096, draw=(8 << 32) | 3, what="eight levels philox")
        assert (got >= count - 300).sum() >= 10, "the philox sample misses the last 300 leaves"
        assert len(np.unique(got >> 24)) >= 3, "the philox sample stays under two level-6 entries"
        u = [int(x) for x in rng.integers(0, 1 << 64, 1000, dtype=np.uint64)]
        assert_samples(t, m, len(u), u=u, what="eight levels injected")
        ends = assert_samples(t, m, 2, u=[0, MASK64], what="eight levels ends")
        assert list(ends) == [0, count - 1] and (m.idx[0], m.idx[-1]) == (0, count - 1)
    finally:
        t.free()


# ----------------------------------------------------------------------------- 5. launch widths
def case_launch_widths(nat, lib, device, count):
    """One update of 2^20 samples (4,096 workgroups, every leaf a duplicate across many of them), a
    second one on top that lowers every leaf, and samples of 65,541 rows (a ragged last workgroup).
    Returns the final (leaf, node, max_q) for the comparison between the engines."""
    t, m = Tree(nat, lib, device, count), Model(count)
    rng = np.random.default_rng(4000 + count)
    M = 1 << 20
    for tt in (t, m):
        tt.fill(0, count, 0, ONE)
    nodes, top = [], ONE
    for lo, hi in ((1.0, 40.0), (0.0, 0.5)):
        idx, p = rng.integers(-3, count + 3, M), rng.uniform(lo, hi, M).astype(np.float32)
        ok = (idx >= 0) & (idx < count)
        assert (~ok).sum() >= 1
        per_leaf = np.bincount(idx[ok], minlength=count)
        assert per_leaf.min() >= (100 if count == 4099 else 1), per_leaf.min()
        for tt in (t, m):
            tt.update(idx, p)
        t.check(m, f"count {count}: update of 2^20 samples in [{lo}, {hi})")
        # the per-leaf maximum, worked out by sorting (not the model's np.maximum.at)
        q = quantise(p)
        order = np.lexsort((q[ok], idx[ok]))
        si, sq = idx[ok][order], q[ok][order]
        last = np.append(si[1:] != si[:-1], True)
        want = np.zeros(count, np.uint32)
        want[si[last]] = sq[last]
        leaf, node, max_q = t.read()
        np.testing.assert_array_equal(leaf[:count], want)
        top = max(top, int(q[ok].max()))
        assert max_q == top
        nodes.append(node.copy())                                     # (on the host engine read() is a view)
    # the second update's clear phase took mass out of every ancestor
    assert (nodes[1][nodes[0] > 0] < nodes[0][nodes[0] > 0]).all() and (nodes[0] > 0).sum() == sum(n for n, _ in shape(count)[2])
    Ms = 65541
    assert_samples(t, m, Ms, draw=(4 << 32) | 9, what=f"count {count} philox")
    u = [int(x) for x in rng.integers(0, 1 << 64, Ms, dtype=np.uint64)]
    assert_samples(t, m, Ms, u=u, what=f"count {count} injected")
    return t.read()


FILL_SHAPES = ((1, 65536), (255, 258), (257, 4095), (4095, 61442), (65521, 16), (65536, 1), (-300, 300))


def case_unaligned_fills(nat, lib, device, count):
    """Fills that start off a workgroup's 256 leaves and run over many workgroups, each with a fresh
    q, then the same shapes in mode 1 after an update has raised max_q.  (first < 0: from the end.)
    Returns the final (leaf, node, max_q)."""
    t, m = Tree(nat, lib, device, count), Model(count)
    rng = np.random.default_rng(5000 + count)
    idx, p = rng.integers(0, count, 5000), rng.uniform(0.0, 8.0, 5000).astype(np.float32)
    for tt in (t, m):
        tt.update(idx, p)
    t.check(m, "scattered start")
    for mode in (0, 1):
        for j, (first, n) in enumerate(FILL_SHAPES):
            first = first % count
            assert first + n <= count
            if mode:                                                  # a new max_q: every fill writes new values
                for tt in (t, m):
                    tt.update([count // 2], [1500.0 + j])
            q = int(rng.integers(0, QMAX + 1))                         # drawn once, given to both
            for tt in (t, m):
                tt.fill(first, n, mode, q)
            t.check(m, f"count {count}: fill({first}, {n}, mode {mode})")
            assert (t.read()[0][first:first + n] == (m.max_q if mode else q)).all()
        if mode == 0:
            for tt in (t, m):
                tt.update([count // 2, 3], [1500.0, 0.25])
            t.check(m, "max_q raised")
            assert m.max_q == 1500 << 20
    assert m.max_q == 1506 << 20
    return t.read()


# ----------------------------------------------------------------------------- 6. the buffer
B, CAP, STEPS = 37, 9, 12                                             # 333 leaves: three levels
BIG = dict(B=8200, cap=9, levels=5, leaf_words=73808, n_update=70000, big_M=4096)   # 73,800 leaves: five levels


def buffer_tree(buf):
    leaf = buf.prio_leaf.cpu().numpy().view(np.uint32)
    node = buf.prio_node.cpu().numpy().view(np.uint64)
    return leaf, node, int(buf.prio_max_q.cpu().numpy().view(np.uint32)[0])


def assert_buffer_tree(buf, m, what):
    leaf, node, max_q = buffer_tree(buf)
    want_leaf, want_node = m.arrays()
    np.testing.assert_array_equal(leaf, want_leaf, err_msg=f"{what}: leaves")
    np.testing.assert_array_equal(node, want_node, err_msg=f"{what}: sums")
    assert max_q == m.max_q, what


def expected_uniform_draw(seed, draw, M, filled, B):
    """replay_cases.expected_draw (philox purpose 6) for a buffer of B envs (that one reads its own B)."""
    m = np.arange(M, dtype=np.uint64)
    c = oph.philox4x32_10(m, draw & 0xFFFFFFFF, draw >> 32, 6 << 24, seed & 0xFFFFFFFF, seed >> 32)
    return oph.uniform_int(filled, c[0]) * B + oph.uniform_int(B, c[1])


def case_buffer(make, variant, na, B=B, cap=CAP, levels=3, leaf_words=336, n_update=150, big_M=37):
    """A prioritized ReplayBuffer over 12 recorded steps of a capacity-`cap` ring of B envs: a recorded
    slot's leaves are max_q, unrecorded slots are 0 and never drawn, update_priorities is the model's
    update of (|p| + eps) ** alpha, sample(M) draws the model's indices, returns what the explicit
    gather of them returns, and weights by the stated formula; then one collect() whose steps wrap
    the ring, so its slots' fill goes out in two parts.  (B = 8,200: five levels, every slot's fill
    starts off a workgroup's 256 leaves and spans 33 workgroups.)"""
    import warehouse
    from replay_cases import place_near_end

    env = make(variant, B, na, seed=SEED)
    place_near_end(env)
    buf = warehouse.ReplayBuffer(env, cap, prioritized=True, alpha=0.6, eps=1e-6)
    assert buf.prio_levels == levels == LEVELS.get(cap * B, levels_of(cap * B))
    assert buf.prio_leaf.numel() == leaf_words and buf.prio_leaf.device == env.state.device
    m = Model(cap * B)
    rng = np.random.default_rng(17)
    assert_buffer_tree(buf, m, "fresh buffer")

    def assert_sample(M, beta, draw, N):
        got = {k: v.clone() for k, v in buf.sample(M, draw=draw, states=True, beta=beta).items()}
        want_idx, want_q = m.sample(philox_draws(SEED, draw, M))
        np.testing.assert_array_equal(got["idx_out"].cpu().numpy(), want_idx)
        np.testing.assert_array_equal(got["prio_q"].cpu().numpy().view(np.uint32), want_q)
        assert want_idx.max() < N and int(buf.prio_total.item()) == m.total()
        again = buf.sample(M, idx=got["idx_out"], states=True)
        assert set(got) == set(again) | {"prio_q", "weights"}
        for k, v in again.items():
            assert torch.equal(v, got[k]), f"{k} differs from the explicit gather"
        w = (want_q.astype(np.float64) / np.float64(m.total()) * N) ** -beta
        w = w / w.max()
        assert got["weights"].dtype == torch.float32
        np.testing.assert_allclose(got["weights"].cpu().numpy(), w, rtol=1e-6, atol=0)

    def update(idx, td, what):
        buf.update_priorities(idx, td)
        p = ((torch.as_tensor(td).to(env.device).abs() + buf.eps) ** buf.alpha).cpu().numpy()
        m.update(idx, p)
        assert_buffer_tree(buf, m, what)

    for s in range(STEPS):
        slot = buf.cursor
        buf.step(env.policy("greedy", 0.3))
        m.fill(slot * B, B, 1)
        assert_buffer_tree(buf, m, f"step {s}")
        leaf = buffer_tree(buf)[0]
        assert (leaf[slot * B:(slot + 1) * B] == m.max_q).all()       # a fresh slot enters at max_q
        assert not leaf[buf.filled * B:].any()                        # slots not yet recorded
        N = len(buf)
        if s in (3, 10):                                              # before and after the ring wraps
            if s == 3:
                got = buf.sample(1000, draw=77)["idx_out"].cpu().numpy()
                assert got.max() < N and len(np.unique(got // B)) == 4   # never an unrecorded slot
            idx = rng.integers(0, N, n_update)
            idx[3] = idx[4]
            td = rng.normal(0.0, 3.0, n_update).astype(np.float32)
            td[:3] = (0.0, 4000.0, -2.5)                              # eps alone; raises max_q; a negative error
            update(idx, td, f"update at step {s}")
            assert m.max_q > ONE
        for M, beta in ((64, 0.4), (big_M, 1.0)):
            assert_sample(M, beta, (s << 8) | M, N)
    assert buf.filled == cap and buf.cursor == STEPS % cap
    # uniform=True and idx=... are the plain paths
    plain = buf.sample(16, draw=5, uniform=True)
    assert "weights" not in plain and "prio_q" not in plain
    want = expected_uniform_draw(SEED, 5, 16, cap, B)
    if B == 37:
        from replay_cases import expected_draw   # (its B is this file's small one: 37)

        np.testing.assert_array_equal(want, expected_draw(SEED, 5, 16, cap))
    np.testing.assert_array_equal(plain["idx_out"].cpu().numpy(), want)
    # every entry below max_q, then a collect() over the end of the ring: its slots enter at max_q
    # through two fills, [cursor, cap) and [0, K - (cap - cursor))
    N, K = len(buf), cap - 1
    update(np.arange(N), rng.uniform(0.0, 2.0, N).astype(np.float32), "update of every entry")
    cursor = buf.cursor
    assert 0 < cap - cursor < K and (buffer_tree(buf)[0][:N] < m.max_q).all()
    buf.collect(K, "greedy", 0.3, observe=False)
    m.fill(cursor * B, (cap - cursor) * B, 1)
    m.fill(0, (K - (cap - cursor)) * B, 1)
    assert_buffer_tree(buf, m, "collect over the end of the ring")
    assert buf.cursor == (cursor + K) % cap and (m.leaf == m.max_q).sum() == K * B
    assert_sample(big_M, 0.4, 0x7000 | big_M, N)


def case_plain_buffer(make):
    """prioritized=False: no tree, the same sample keys as before, update_priorities raises."""
    import pytest
    import warehouse

    env = make("small", 5, 4, seed=3)
    env.reset()
    buf = warehouse.ReplayBuffer(env, 3)
    assert buf.prioritized is False
    assert not [a for a in vars(buf) if "prio" in a and a != "prioritized"] and not hasattr(buf, "_tree")
    buf.step(env.policy())
    assert set(buf.sample(4)) == {"obs", "next_obs", "actions", "rewards", "dones", "n", "idx_out"}
    with pytest.raises(ValueError, match="prioritized"):
        buf.update_priorities([0], [1.0])
    with pytest.raises(ValueError):
        warehouse.ReplayBuffer(env, 3, prioritized=True, alpha=-1.0)
    pb = warehouse.ReplayBuffer(env, 3, prioritized=True)
    with pytest.raises(ValueError):
        pb.update_priorities([0, 1], [1.0])
    pb.step(env.policy())
    out = pb.sample(0)
    assert out["prio_q"].shape == (0,) and out["weights"].shape == (0,)


# ----------------------------------------------------------------------------- 7. refusals
def case_refusals(nat, lib, host: bool):
    """The refusals of wh_replay_prio_*: codes of one library as a list (the caller compares the two
    libraries' lists).  On the host engine every pointer is a real sentinel-filled buffer that must
    stay untouched; on the device library dummies that a refused or empty call never dereferences."""
    count, M = 333, 5
    lw, nw, levels = shape(count)
    keep = []

    def mem(nbytes):
        if not host:
            keep.append(None)
            return 4096 * len(keep)
        t = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8)
        keep.append(t)
        return t.data_ptr()

    tree = dict(leaf=mem(4 * lw), node=mem(8 * nw), max_q=mem(4), count=count)
    idx, p, u, idx_out, q_out, total_out = mem(8 * M), mem(4 * M), mem(8 * M), mem(8 * M), mem(4 * M), mem(8)

    def tp(tree_):
        return None if tree_ is None else ctypes.byref(nat.WhReplayPrio(**tree_))

    def fill(tree_=tree, first=0, n=0, mode=0, q=ONE):
        return lib.wh_replay_prio_fill(tp(tree_), first, n, mode, q, None)

    def upd(tree_=tree, M_=0, idx_=idx, p_=p):
        return lib.wh_replay_prio_update(tp(tree_), M_, idx_, p_, None)

    def smp(tree_=tree, M_=0, idx_out_=idx_out):
        return lib.wh_replay_prio_sample(tp(tree_), M_, u, 1, 2, idx_out_, q_out, total_out, None)

    def qry(count_):
        a, b, c = ctypes.c_int64(-7), ctypes.c_int64(-7), ctypes.c_int32(-7)
        rc = lib.wh_replay_prio_query(count_, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
        assert rc == nat.WH_OK or (a.value, b.value, c.value) == (-7, -7, -7)
        return rc

    E, OK = nat.WH_EINVAL, nat.WH_OK
    table = [("query: count 0", qry(0), E), ("query: count -1", qry(-1), E), ("query: count 2^31 + 1", qry((1 << 31) + 1), E),
             ("query: count 2^31", qry(1 << 31), OK), ("query: count 1", qry(1), OK)]
    a, b, c = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
    assert lib.wh_replay_prio_query(1 << 31, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == OK
    assert (a.value, c.value) == (1 << 31, 8) and b.value == sum(max(16, 1 << s) for s in (27, 23, 19, 15, 11, 7, 3, 0))
    assert lib.wh_replay_prio_query(17, None, None, None) == OK
    for name, call in (("fill", fill), ("update", upd), ("sample", smp)):
        table += [
            (f"{name}: NULL tree", call(tree_=None), E),
            (f"{name}: NULL leaf", call(tree_=dict(tree, leaf=None)), E),
            (f"{name}: NULL node", call(tree_=dict(tree, node=None)), E),
            (f"{name}: NULL max_q", call(tree_=dict(tree, max_q=None)), E),
            (f"{name}: count 0", call(tree_=dict(tree, count=0)), E),
            (f"{name}: count -5", call(tree_=dict(tree, count=-5)), E),
            (f"{name}: count 2^31 + 1", call(tree_=dict(tree, count=(1 << 31) + 1)), E),
        ]
    table += [
        ("fill: first -1", fill(first=-1, n=1), E),
        ("fill: first = count, n = 1", fill(first=count, n=1), E),
        ("fill: first > count", fill(first=count + 1), E),
        ("fill: n -1", fill(n=-1), E),
        ("fill: n > count", fill(n=count + 1), E),
        ("fill: first + n > count", fill(first=300, n=34), E),
        ("fill: first + n overflows", fill(first=1, n=(1 << 63) - 1), E),
        ("fill: mode 2", fill(mode=2), E),
        ("fill: mode -1", fill(mode=-1), E),
        ("fill: q 2^31", fill(q=1 << 31), E),
        ("fill: bad mode before a bad tree", fill(mode=2, tree_=None), E),
        ("fill: n = 0", fill(), OK),
        ("fill: n = 0 at the end", fill(first=count), OK),
        ("fill: n = 0, mode 1", fill(mode=1), OK),
        ("update: M -1", upd(M_=-1), E),
        ("update: NULL idx", upd(M_=M, idx_=None), E),
        ("update: NULL p", upd(M_=M, p_=None), E),
        ("update: M = 0", upd(), OK),
        ("update: M = 0, NULL idx and p", upd(idx_=None, p_=None), OK),
        ("sample: M -1", smp(M_=-1), E),
        ("sample: NULL idx_out", smp(M_=M, idx_out_=None), E),
        ("sample: M = 0", smp(), OK),
        ("sample: M = 0, NULL idx_out", smp(idx_out_=None), OK),
    ]
    for what, rc, want in table:
        assert rc == want, f"{what}: got {rc}, expected {want}"
    for t in keep:
        assert t is None or bool((t == 0xA5).all()), "a refused (or empty) call wrote to a buffer"
    return [(what, rc) for what, rc, _ in table]
