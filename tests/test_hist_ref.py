"""tests/hist_ref.py against hand-worked cases: the bin rule of kacc_group_hist pinned down."""

import numpy as np

from group_ref import KACC_GROUP_NONE
from hist_ref import bounds_valid, group_hist

READ_ERROR = 0x1


def f64(*values):
    return np.array(values, dtype=np.float64).view(np.uint64)


def power_hist(powers, bounds, group=None, n_groups=1, row_off=None, status=None, mask=None):
    """One zone, row i at slot i."""
    n = len(powers)
    return group_hist(np.array(powers, dtype=np.float64), True, 1, 0, [0, n] if row_off is None else row_off,
                      np.arange(n, dtype=np.uint32), status, mask, group, n_groups, bounds)


def test_a_value_equal_to_a_bound_lands_at_or_below_it():
    b, cum, s, nan, uns = power_hist([1.0, 2.0, 2.0, 3.0, 0.5], f64(1.0, 2.0))
    assert b.tolist() == [[2, 2, 1]]  # 0.5 and 1.0 | 2.0 twice | 3.0
    assert cum.tolist() == [[2, 4, 5]]
    assert s.tolist() == [int(8.5 * 4096)] and nan.tolist() == [0] and uns.tolist() == [0]


def test_the_zeros_share_a_key():
    for bound in (0.0, -0.0):
        b, cum, *_ = power_hist([-0.0, 0.0, -1e-300, 5e-324], f64(bound))
        assert b.tolist() == [[3, 1]]  # both zeros and the negative | the smallest denormal
    assert not bounds_valid(f64(0.0, -0.0), True) and not bounds_valid(f64(-0.0, 0.0), True)


def test_a_nan_goes_to_out_nan_only():
    nans = np.array([0x7FF8000000000000, 0xFFF8000000000001, 0x7FF0000000000001], dtype=np.uint64).view(np.float64)
    b, cum, s, nan, uns = power_hist([*nans, 1.0], f64(-np.inf, 0.0, np.inf))
    assert b.tolist() == [[0, 0, 1, 0]] and cum.tolist() == [[0, 0, 1, 1]]
    assert nan.tolist() == [3] and uns.tolist() == [0] and s.tolist() == [4096]
    assert not bounds_valid(f64(np.nan), True) and not bounds_valid(f64(1.0, np.nan), True)


def test_infinities_and_huge_powers_are_binned_and_unsummed():
    b, cum, s, nan, uns = power_hist([np.inf, -np.inf, 2.0 ** 50, 1e300, 1.5, np.nextafter(2.0 ** 50, 0)],
                                     f64(-np.inf, 2.0, np.inf))
    assert b.tolist() == [[1, 1, 4, 0]]  # -Inf | 1.5 | 2^50, 1e300, just below 2^50, +Inf (<= the +Inf bound)
    b2, *_ = power_hist([np.inf, 1.0], f64(2.0))
    assert b2.tolist() == [[1, 1]]  # +Inf is in the last bin
    assert uns.tolist() == [4] and nan.tolist() == [0]
    want = (int(1.5 * 4096) + int(np.nextafter(2.0 ** 50, 0) * 4096)) % 2 ** 64
    assert s.tolist() == [want]
    assert cum[0, -1] == 6


def test_negative_powers_against_negative_bounds():
    b, cum, s, nan, uns = power_hist([-3.0, -1.5, -1.0, -0.25, 0.0, 2.0], f64(-2.0, -1.5, -0.5))
    assert b.tolist() == [[1, 1, 1, 3]]  # -3 | -1.5 (equal) | -1 | -0.25, 0, 2
    assert s.view(np.int64).tolist() == [int(-3.75 * 4096)]
    assert bounds_valid(f64(-2.0, -1.5), True) and not bounds_valid(f64(-1.5, -2.0), True)


def test_energy_keys_are_the_values():
    top = 2 ** 64 - 1
    e = np.array([0, 5, top, top, 7], dtype=np.uint64)
    args = (e, False, 1, 0, [0, 5], np.arange(5, dtype=np.uint32), None, None, None, 1)
    b, cum, s, nan, uns = group_hist(*args, np.array([5, top - 1], dtype=np.uint64))
    assert b.tolist() == [[2, 1, 2]]
    assert s.tolist() == [(12 + 2 * top) % 2 ** 64] and nan.tolist() == [0] and uns.tolist() == [0]
    b, *_ = group_hist(*args, np.array([top], dtype=np.uint64))
    assert b.tolist() == [[5, 0]]  # 2^64 - 1 is at its own bound, nothing is above it
    assert not bounds_valid(np.array([5, 5], dtype=np.uint64), False)
    assert not bounds_valid(np.zeros(0, dtype=np.uint64), False)
    assert bounds_valid(np.arange(64, dtype=np.uint64), False) and not bounds_valid(np.arange(65, dtype=np.uint64), False)


def test_groups_none_ids_unlisted_nodes_and_the_count_column():
    powers = [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, np.nan]
    group = np.array([0, 1, KACC_GROUP_NONE, 1, 0, 1, 1], dtype=np.uint32)
    row_off = [0, 2, 5, 7]  # node 1 holds rows 2..4
    b, cum, s, nan, uns = power_hist(powers, f64(2.0, 4.5), group, 3, row_off)
    assert b.tolist() == [[1, 0, 1], [1, 1, 1], [0, 0, 0]]
    assert cum[:, -1].tolist() == [2, 3, 0] and nan.tolist() == [0, 1, 0]
    assert s.tolist() == [6 * 4096, 12 * 4096, 0]
    # node 1 unlisted by the mask, or by a read error
    for status, mask in ((None, [1, 0, 7]), ([0, READ_ERROR, 0], None)):
        b, cum, s, nan, uns = power_hist(powers, f64(2.0, 4.5), group, 3, row_off, status, mask)
        assert b.tolist() == [[1, 0, 0], [1, 0, 1], [0, 0, 0]]
        assert cum[:, -1].tolist() == [1, 2, 0] and nan.tolist() == [0, 1, 0]
    # an id of n_groups and a slot past the table are left out
    bad = group.copy()
    bad[0] = 3
    b, *_ = power_hist(powers, f64(2.0, 4.5), bad, 3, row_off)
    assert b.tolist() == [[0, 0, 1], [1, 1, 1], [0, 0, 0]]
    words = np.arange(7, dtype=np.uint32)
    words[1] = 7
    b, *_ = group_hist(np.array(powers), True, 1, 0, row_off, words, None, None, group, 3, f64(2.0, 4.5))
    assert b.tolist() == [[1, 0, 1], [0, 1, 1], [0, 0, 0]]
