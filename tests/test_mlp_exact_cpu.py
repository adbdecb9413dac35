"""What makes tests/test_gpu_mlp_exact.py mean something, checked without a GPU on the generator and
the float64 reference of tests/mlp_exact_cases.py: the sums stay exact in f32, every value is what a
bf16 can hold (or is planted not to be), the summation order cannot matter, the integer-code rounder
is torch's, the cases reach the rounding ties and the argmax tie, and every modelled kernel bug moves
at least one logit of the test rows.

Measured here (printed by the tests; run with -s):
  worst sum |w||h| + |b| in grains of its row, over every case and both precisions (limit 2^24 =
  1.68e7): layer 0 2.7e4, layer 1 2.0e5, layer 2 5.7e6 -- the rounding row, whose grain is 2^-2; on
  the integer rows 2.0e3, 8.2e3 and 1.3e5.
  exact ties at the hidden layers of the 300-row cases (down to even + up to even): layer 0 between
  331 + 363 and 807 + 762, layer 1 between 2914 + 2932 and 7308 + 7491; live hidden units 48-51 %;
  units dead in every row: at most 4 at layer 0 (three of them the negative planted b0), 2 at layer 1.
  rows whose maximum is the tied pair: small 38, medium 50, large 93 of 300; distinct argmax 6-7.
  swaps of two unequal weights seen: small 599, medium 600, large 600 of 600."""
import numpy as np
import pytest

import mlp_exact_cases as mx

PRECISIONS = ("bf16", "f32")


def ids(c):
    return "-".join(str(v) for v in c)


@pytest.mark.parametrize("case", mx.CASES, ids=ids)
def test_sums_stay_exact_in_f32(case):
    for precision in PRECISIONS:
        w, x, ref = mx.case(*case, precision)
        print(ids(case), precision, "worst sums in grains, per layer:", ["%.3g" % s for s in ref["worst"]])
        assert max(ref["worst"]) < mx.LIMIT, (case, precision, ref["worst"])
        # the logits are whole grains
        g = mx.grain(x)[:, None]
        assert np.array_equal(ref["logits"] / g, np.round(ref["logits"] / g))
    # the integer rows alone
    ints = mx.grain(x) == 1.0
    if ints.any():
        print(ids(case), "integer rows:", ["%.3g" % s for s in mx.reference(w, x[ints], "bf16")["worst"]])


@pytest.mark.parametrize("case", mx.CASES, ids=ids)
def test_values_are_representable(case):
    variant, seed, rows = case
    w, x = mx.network(variant, seed), mx.inputs(variant, seed, rows)
    for k in mx.KEYS:
        assert np.array_equal(w[k], np.round(w[k])), k
        if k in ("w0", "w1", "w2"):                   # (b1 and b2 stay f32 in the blob, b0 is hi + lo)
            assert np.array_equal(mx.to_bf16(w[k]), w[k]), f"{k} does not fit bf16"
    hi, lo = mx.split_b0(w["b0"])
    assert np.array_equal(hi.astype(np.float64) + lo.astype(np.float64), w["b0"].astype(np.float64))
    assert int((lo != 0).sum()) >= 8
    assert tuple(w["b0"][:8]) == (257, -259, 1027, -515, 300, 387, -33, 641)
    # the generator's ranges
    assert set(np.unique(w["w0"])) <= {-3, -2, -1, 0, 1, 2, 3} and 0.45 < (w["w0"] != 0).mean() < 0.55
    assert set(np.unique(w["w1"])) <= {-2, -1, 0, 1, 2} and 20 < (w["w1"] != 0).sum(axis=1).mean() < 28
    assert set(np.unique(w["w2"])) == {-1, 1}
    assert np.array_equal(w["w2"][mx.TIED[0]], w["w2"][mx.TIED[1]]) and w["b2"][mx.TIED[0]] == w["b2"][mx.TIED[1]]
    assert len({w["w2"][o].tobytes() for o in range(9)}) == 8
    planted = w["w1"][:, :len(mx.B0_PLANTED)] @ np.maximum(np.array(mx.B0_PLANTED, np.float32), 0)
    assert np.abs(w["b1"] + planted).max() <= 256 + 2 and not (w["b1"] % 4).any() and np.abs(w["b2"]).max() <= 8
    # inputs: only the rounding row does not fit bf16, and it rounds in both directions
    fits = (mx.to_bf16(x) == x).all(axis=1)
    rr = mx.rounding_row(rows)
    assert not fits[rr] and fits[np.arange(rows) != rr].all()
    assert set(mx.INT_ROUNDED + mx.FRAC_ROUNDED) <= set(x[rr].tolist())
    others = np.delete(x, rr, axis=0)
    assert others.size == 0 or (np.abs(others).max() <= 9 and np.array_equal(others, np.round(others)))
    if rows > 1:
        assert not x[rows - 1].any()
    if rows >= 8:
        binary = ((x == 0) | (x == 1)).all(axis=1)
        assert binary.sum() >= rows // 4


def test_planted_values_round_in_both_directions():
    v = np.array(mx.INT_ROUNDED + mx.FRAC_ROUNDED, np.float32)
    want = np.array([256, 260, -256, -260, 64, 65, -64, -65], np.float32)
    assert np.array_equal(mx.to_bf16(v), want)
    down, up = mx.ties(np.abs(v))
    assert down == 4 and up == 4


@pytest.mark.parametrize("case", mx.CASES, ids=ids)
def test_summation_order_cannot_matter(case):
    """float32, one k at a time in three shuffled orders: the bits of the float64 reference."""
    for precision in PRECISIONS:
        w, x, ref = mx.case(*case, precision)
        for shuffle in range(3):
            got = mx.shuffled_f32(w, x, precision, seed=shuffle)
            assert got.dtype == np.float32
            assert np.array_equal(got.astype(np.float64), ref["logits"]), (case, precision, shuffle)


def test_rounder_is_torchs():
    import torch

    rng = np.random.default_rng(3)
    planted = np.array(mx.INT_ROUNDED + mx.FRAC_ROUNDED + mx.B0_PLANTED +
                       (1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 0.0, -0.0, 1.0), np.float32)
    bits = rng.integers(0, 1 << 31, 2000).astype(np.uint32)
    exact_ties = ((bits & np.uint32(0xFFFF0000)) | np.uint32(0x8000)).view(np.float32)
    rnd = np.concatenate([(rng.standard_normal(6000) * 300).astype(np.float32),
                          rng.integers(-70000, 70000, 3000).astype(np.float32), exact_ties])
    rnd = rnd[np.isfinite(rnd)]
    assert rnd.size >= 10000
    for v in (planted, rnd):
        want = torch.as_tensor(v).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(mx.bf16_bits(v), want)
        assert np.array_equal(mx.to_bf16(v), torch.as_tensor(v).to(torch.bfloat16).to(torch.float32).numpy())


def test_fragments_are_the_rows_in_operand_order():
    """fragments() against a per-element loop of the layout's definition."""
    in_dim = 37
    x = mx.inputs("small", 5, 33)
    fr = mx.fragments(x, in_dim)
    kq = 3
    assert fr.shape == (2, kq, 64, 8) and fr.dtype == np.uint16
    one, rounded = mx.bf16_bits(np.float32(1.0)), mx.bf16_bits(x)
    for tile in range(2):
        for q in range(kq):
            for lane in range(64):
                for j in range(8):
                    row, k = 32 * tile + (lane & 31), 16 * q + 8 * (lane >> 5) + j
                    want = (rounded[row, k] if row < 33 else 0) if k < in_dim else one if k < in_dim + 2 else 0
                    assert fr[tile, q, lane, j] == want, (tile, q, lane, j)


@pytest.mark.parametrize("variant", mx.VARIANTS)
def test_coverage_of_the_300_row_case(variant):
    for precision in PRECISIONS:
        w, x, ref = mx.case(variant, mx.SEED[variant], 300, precision)
        for i in (0, 1):
            pre = ref[f"pre{i}"].astype(np.float32)
            assert np.array_equal(pre.astype(np.float64), ref[f"pre{i}"])
            down, up = mx.ties(pre)
            live = float((pre > 0).mean())
            print(variant, precision, "layer", i, "ties down / up", down, up, "live %.3f" % live)
            assert down + up >= 100 and down > 0 and up > 0
            assert 0.3 <= live <= 0.7
            # a unit that is dead in every row hides its weights: the negative planted b0, few others
            dead = int((pre <= 0).all(axis=0).sum())
            print(variant, precision, "layer", i, "units dead in every row", dead, "of", pre.shape[1])
            assert dead <= 4
        z = ref["logits"]
        tied_max = int((z.max(axis=1) == z[:, mx.TIED[0]]).sum())
        distinct = np.unique(ref["actions"]).size
        print(variant, precision, "rows whose maximum is the tied pair", tied_max, "distinct argmax", distinct)
        assert np.array_equal(z[:, mx.TIED[0]], z[:, mx.TIED[1]])
        assert tied_max >= 20 and distinct >= 3
        # on those rows the first of the pair wins, never the second
        assert (ref["actions"] == mx.TIED[0]).sum() == tied_max and not (ref["actions"] == mx.TIED[1]).any()
        assert np.array_equal(ref["actions"], np.argmax(z, axis=1))


@pytest.mark.parametrize("variant", mx.VARIANTS)
def test_every_modelled_bug_moves_a_logit(variant):
    w, x, ref = mx.case(variant, mx.SEED[variant], 300, "bf16")
    z = ref["logits"]

    def moved(what, other):
        n = int((other["logits"] != z).any(axis=1).sum())
        print(variant, what, "changes", n, "of 300 rows")
        assert n > 0, what

    moved("hidden truncated", mx.reference(w, x, "bf16", hidden=mx.trunc_bf16))
    moved("hidden ties away from zero", mx.reference(w, x, "bf16", hidden=mx.away_bf16))
    moved("b0 without lo", mx.reference(w, x, "bf16", drop_lo=True))
    moved("x truncated", mx.reference(w, x, "bf16", xround=mx.trunc_bf16))
    moved("x ties away from zero", mx.reference(w, x, "bf16", xround=mx.away_bf16))
    rng = np.random.default_rng(11)
    for k in ("b1", "b2"):
        for precision in PRECISIONS:
            b = w[k].copy()
            b[rng.integers(b.size)] += 1
            base = mx.case(variant, mx.SEED[variant], 300, precision)[2]["logits"]
            assert (mx.reference(dict(w, **{k: b}), x, precision)["logits"] != base).any(), (k, precision)
    # the f32 network must see a rounded x
    z32 = mx.case(variant, mx.SEED[variant], 300, "f32")[2]["logits"]
    assert (mx.reference(w, mx.to_bf16(x), "f32")["logits"] != z32).any()
    # 200 swaps of two unequal elements per matrix
    seen = total = 0
    for k in ("w0", "w1", "w2"):
        hit = 0
        for n in range(200):
            m = w[k].copy()
            flat = m.reshape(-1)
            i = int(rng.integers(flat.size))
            j = int(rng.integers(flat.size))
            while flat[j] == flat[i]:
                j = int(rng.integers(flat.size))
            flat[i], flat[j] = flat[j], flat[i]
            other = mx.logits_with(w, ref, k, m)
            if n < 3:                                 # the short cut is the whole reference
                assert np.array_equal(other, mx.reference(dict(w, **{k: m}), x, "bf16")["logits"])
            hit += bool((other != z).any())
        print(variant, k, "swaps seen", hit, "of 200")
        assert hit >= 198
        seen, total = seen + hit, total + 200
    print(variant, "swaps seen", seen, "of", total)
    assert seen >= 0.99 * total
