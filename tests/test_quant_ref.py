"""tests/quant_ref.py against a brute-force restatement in plain Python: a sorted list per group and
Prometheus' quantile formula in Python floats (the same IEEE doubles), bit for bit."""

import math
import struct

import numpy as np

from group_ref import KACC_GROUP_NONE
from quant_ref import EMPTY_NAN, group_quantiles, key_bits, phi_valid
from top_ref import sort_key

PHI = [0.0, 1.0, 0.5, 0.99, 1.0 / 3.0]
MASK64 = (1 << 64) - 1


def bits_of(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def float_of(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def py_key(bits, is_power):
    """The header's key of one value, on Python ints; None for a NaN power."""
    if not is_power:
        return bits
    mag = bits & (MASK64 >> 1)
    if mag > 0x7FF0000000000000:
        return None
    if mag == 0:
        return 1 << 63
    return (~bits & MASK64) if bits >> 63 else bits | 1 << 63


def py_bits(key, is_power):
    if not is_power:
        return key
    return key & (MASK64 >> 1) if key >> 63 else ~key & MASK64


def brute(bits, is_power, group, n_groups, phi):
    """The six outputs as lists of Python ints (weight and value as bits)."""
    count, nan, lo, hi, weight, value = [], [], [], [], [], []
    for g in range(n_groups):
        keys = [py_key(int(b), is_power) for b, gr in zip(bits, group) if gr == g]
        nan.append(sum(k is None for k in keys))
        ranked = sorted(k for k in keys if k is not None)
        n = len(ranked)
        count.append(n)
        for f in phi:
            if n == 0:
                lo.append(0), hi.append(0), weight.append(0), value.append(int(EMPTY_NAN))
                continue
            rank = f * float(n - 1)
            lower = math.floor(rank)
            upper = min(n - 1, lower + 1)
            w = rank - math.floor(rank)
            b_lo, b_hi = py_bits(ranked[lower], is_power), py_bits(ranked[upper], is_power)
            x_lo, x_hi = (float_of(b_lo), float_of(b_hi)) if is_power else (float(b_lo), float(b_hi))
            lo.append(b_lo), hi.append(b_hi), weight.append(bits_of(w))
            value.append(bits_of(x_lo * (1.0 - w) + x_hi * w))
    return count, nan, lo, hi, weight, value


def flat(out):
    c, n, lo, hi, w, v = out
    u = lambda x: [int(i) for i in np.ascontiguousarray(x).view(np.uint64).reshape(-1)]  # noqa: E731
    return u(c), u(n), u(lo), u(hi), u(w), u(v)


def random_powers(rng, n):
    v = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 9, n)
    special = np.array([0.0, -0.0, 1.5, -1.5, np.inf, -np.inf, 1e300, -1e-300])
    pick = rng.random(n) < 0.4
    v[pick] = special[rng.integers(0, special.size, int(pick.sum()))]
    bits = v.view(np.uint64).copy()
    nans = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)
    pick = rng.random(n) < 0.05
    bits[pick] = nans[rng.integers(0, nans.size, int(pick.sum()))]
    return bits


def run_case(bits, is_power, group, n_groups, phi=PHI):
    n = bits.size
    table = bits.view(np.float64) if is_power else bits
    row_off = np.array([0, n], dtype=np.uint32)
    slots = np.arange(n, dtype=np.uint32)
    got = group_quantiles(table, is_power, 1, 0, row_off, slots, None, None, group, n_groups, phi)
    want = brute(bits, is_power, [0] * n if group is None else group, n_groups, phi)
    for name, a, b in zip(("count", "nan", "lo", "hi", "weight", "value"), flat(got), want):
        assert a == b, name
    return got


def test_random_rows_equal_the_brute_force():
    rng = np.random.default_rng(5)
    n = 400
    for is_power in (True, False):
        bits = random_powers(rng, n) if is_power else rng.integers(0, 1 << 63, n).astype(np.uint64) << np.uint64(1)
        bits[rng.random(n) < 0.3] = bits[0]  # duplicates
        group = rng.integers(0, 6, n).astype(np.uint32)
        group[rng.random(n) < 0.05] = KACC_GROUP_NONE
        # groups 6, 7, 8 hold 0, 1 and 2 ranked rows (and a NaN row each for a power)
        group[group == 6] = 0
        bits = np.concatenate([bits, np.array([bits[1], bits[2], bits[3]], dtype=np.uint64)])
        group = np.concatenate([group, np.array([7, 8, 8], dtype=np.uint32)])
        if is_power:
            bits = np.concatenate([bits, np.full(3, 0x7FF8000000000123, dtype=np.uint64)])
            group = np.concatenate([group, np.array([6, 7, 8], dtype=np.uint32)])
            bits[-6:-3] = np.array([1.5, -2.5, 0.0]).view(np.uint64)
        c, nn, lo, hi, w, v = run_case(bits, is_power, group, 9)
        assert list(c[6:]) == [0, 1, 2]
        assert v.view(np.uint64)[6, 0] == EMPTY_NAN and not w[6].any() and not lo[6].any()
        if is_power:
            assert list(nn[6:]) == [1, 1, 1] and nn.sum() > 3
            assert (np.isinf(v)).any() or np.isnan(v[:6]).any()  # the ±Inf rows reached a result


def test_group_none_and_the_single_group():
    rng = np.random.default_rng(9)
    bits = random_powers(rng, 200)
    run_case(bits, True, None, 1)
    run_case(rng.integers(0, 50, 200).astype(np.uint64), False, None, 1, phi=[1.0 / 3.0])


def test_the_inverse_round_trips_every_value_but_minus_zero():
    rng = np.random.default_rng(2)
    vals = np.concatenate([rng.standard_normal(500) * 10.0 ** rng.integers(-300, 300, 500),
                           [0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 1.7976931348623157e308]])
    back = key_bits(sort_key(vals, True), True)
    want = vals.view(np.uint64).copy()
    want[vals == 0] = 0  # -0.0 comes back as +0.0
    np.testing.assert_array_equal(back, want)
    e = rng.integers(0, 1 << 63, 100).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    np.testing.assert_array_equal(key_bits(sort_key(e, False), False), e)


def test_phi_0_is_the_minimum_and_phi_1_the_maximum():
    rng = np.random.default_rng(3)
    vals = rng.standard_normal(300) * 100.0
    group = rng.integers(0, 4, 300).astype(np.uint32)
    c, _, lo, hi, w, v = run_case(vals.view(np.uint64).copy(), True, group, 4, phi=[0.0, 1.0])
    for g in range(4):
        mine = vals[group == g]
        assert lo.view(np.float64)[g, 0] == mine.min() == v[g, 0]
        assert lo.view(np.float64)[g, 1] == mine.max() == hi.view(np.float64)[g, 1] == v[g, 1]
    assert not w.any()


def test_phi_validity():
    assert phi_valid([0.0, 1.0]) and phi_valid([0.5] * 8)
    for bad in ([], [0.5] * 9, [np.nan], [-0.1], [1.0000001], [0.5, 2.0]):
        assert not phi_valid(bad)
