"""tests/derive_ref.py pinned on the guard's truth table, worked out by hand (no GPU)."""

import math

import numpy as np

from derive_ref import assert_power_equal, derived_power

NAN = float("nan")


def one(ratio, node, aE, aP, cd, nodes=1):
    """Power bits of one slot in a one-zone fleet whose node 0 has these values."""
    p = derived_power([ratio], [node], [aE] * nodes, [aP] * nodes, [cd] * nodes, nodes, 1)
    assert p.shape == (1,) and p.dtype == np.float64
    return p.view(np.uint64)[0]


def bits(x):
    return np.array([x], dtype=np.float64).view(np.uint64)[0]


def test_guard_truth_table():
    assert one(0.5, 0, 7, 3.0, 2.0) == bits(1.5)            # every term holds
    assert one(0.5, 0, 0, 3.0, 2.0) == bits(0.0)            # activeEnergy == 0
    assert one(0.5, 0, 7, 3.0, 0.0) == bits(0.0)            # nodeCPUTimeDelta == 0
    assert one(0.5, 0, 7, 0.0, 2.0) == bits(0.0)            # ActivePower == 0
    assert one(0.5, 1, 7, 3.0, 2.0) == bits(0.0)            # node == nodes: no such node
    assert one(0.5, 0xFFFFFFFF, 7, 3.0, 2.0) == bits(0.0)
    assert one(0.5, 1, 7, 3.0, 2.0, nodes=2) == bits(1.5)   # the last node


def test_minus_zero_fails_the_guard_and_gives_plus_zero():
    assert one(0.5, 0, 7, 3.0, -0.0) == bits(0.0)
    assert one(0.5, 0, 7, -0.0, 2.0) == bits(0.0)
    assert one(-0.5, 0, 7, -0.0, 2.0) == bits(0.0) != bits(-0.0)
    assert one(-0.5, 0, 0, 3.0, 2.0) == bits(0.0)


def test_nan_passes_the_guard():
    assert one(0.5, 0, 7, 3.0, NAN) == bits(1.5)            # a NaN cpu delta: NaN != 0
    assert math.isnan(derived_power([0.5], [0], [7], [NAN], [2.0], 1, 1)[0])
    assert math.isnan(derived_power([NAN], [0], [7], [3.0], [2.0], 1, 1)[0])
    assert one(NAN, 0, 0, 3.0, 2.0) == bits(0.0)            # behind a failed guard the ratio is not read


def test_the_product_keeps_its_sign_and_range():
    assert one(-0.0, 0, 7, 3.0, 2.0) == bits(-0.0)          # the result may be -0.0
    assert one(0.0, 0, 7, -3.0, 2.0) == bits(-0.0)
    assert one(0.0, 0, 7, 3.0, 2.0) == bits(0.0)
    assert one(5e-324, 0, 7, 0.5, 2.0) == bits(0.0)         # a subnormal halves to zero (ties to even)
    assert one(5e-324, 0, 7, 3.0, 2.0) == bits(1.5e-323)
    assert one(1e300, 0, 7, 1e300, 2.0) == bits(float("inf"))
    assert one(float("inf"), 0, 7, -2.0, 2.0) == bits(float("-inf"))
    assert one(-2.5, 0, 1 << 63, 4.0, -1.0) == bits(-10.0)


def test_layout_slot_major_zones_minor():
    # 2 nodes x 2 zones; aP = [[10, 20], [30, 0]], activeEnergy = [[1, 0], [1, 1]], cpu delta = [1, 1]
    p = derived_power([2.0, 3.0, 4.0], [1, 0, 2], [1, 0, 1, 1], [10.0, 20.0, 30.0, 0.0], [1.0, 1.0], 2, 2)
    assert p.tolist() == [60.0, 0.0, 30.0, 0.0, 0.0, 0.0]


def test_assert_power_equal_masks_by_the_reference_only():
    assert_power_equal([1.0, NAN, -0.0], [1.0, NAN, -0.0])
    for got, want in (([NAN], [1.0]), ([1.0], [NAN]), ([0.0], [-0.0])):
        try:
            assert_power_equal(got, want)
        except AssertionError:
            continue
        raise AssertionError((got, want))
