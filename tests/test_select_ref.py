"""tests/select_ref.py (the rule of kacc_select_above in numpy) against values written out here.

Four nodes (3, 2, 0 and 3 rows), Z = 2, eight slots.  Zone 1 of the power table holds one value of
every special kind; the energy of slot s in zone z is 100 s + z.
"""

import numpy as np

from select_ref import select_above, threshold_key

Z = 2
ROW_OFF = [0, 3, 5, 5, 8]
NEW = 0x80000000  # KACC_SLOT_NEW: ignored
SLOT_WORDS = np.array([5, 2 | NEW, 7, 0, 1, 3, 4, 6], dtype=np.uint32)
DENORM = 5e-324  # bits 1
#                 slot 0   1     2    3     4       5    6       7
P1 = np.array([np.nan, -0.0, 0.0, -2.5, np.inf, 1.5, DENORM, 3.0])
POWER = np.stack([np.arange(8) * 10.0, P1], axis=1).reshape(-1)
ENERGY = np.array([[100 * s, 100 * s + 1] for s in range(8)], dtype=np.uint64).reshape(-1)
# the rows' zone-1 powers: 1.5, +0.0, 3.0 | NaN, -0.0 | | -2.5, +Inf, 5e-324


def bits(x):
    return int(np.array([x], dtype=np.float64).view(np.uint64)[0])


def run(thr, by_power=True, zone=1, status=None, mask=None, cap=100):
    return select_above(ENERGY, POWER, Z, zone, by_power, ROW_OFF, SLOT_WORDS, status, mask, thr, cap)


def rows_and_off(out):
    return out[1].tolist(), out[0].tolist()


def test_threshold_keys():
    top = 1 << 63
    assert threshold_key(bits(np.nan), True) == 0
    assert threshold_key(bits(0.0), True) == top == threshold_key(bits(-0.0), True)
    assert threshold_key(1, True) == top | 1
    assert threshold_key(bits(-2.5), True) == (~bits(-2.5)) & (2**64 - 1)
    assert threshold_key(12345, False) == 12345


def test_power_thresholds_of_every_special_kind():
    # NaN: every listed row, the NaN row included
    assert rows_and_off(run(bits(np.nan))) == ([0, 1, 2, 3, 4, 5, 6, 7], [0, 3, 5, 5, 8])
    # +0.0 and -0.0: every non-negative power, both zeros, no NaN
    for zero in (0.0, -0.0):
        assert rows_and_off(run(bits(zero))) == ([0, 1, 2, 4, 6, 7], [0, 3, 4, 4, 6])
    # the smallest denormal: strictly positive
    assert rows_and_off(run(1)) == ([0, 2, 6, 7], [0, 2, 2, 2, 4])
    # a present value: >= keeps the equal key
    assert rows_and_off(run(bits(1.5))) == ([0, 2, 6], [0, 2, 2, 2, 3])
    # a negative: every number, not the NaN
    assert rows_and_off(run(bits(-2.5))) == ([0, 1, 2, 4, 5, 6, 7], [0, 3, 4, 4, 7])
    assert rows_and_off(run(bits(-2.0))) == ([0, 1, 2, 4, 6, 7], [0, 3, 4, 4, 6])
    # +Inf
    assert rows_and_off(run(bits(np.inf))) == ([6], [0, 0, 0, 0, 1])


def test_outputs_carry_all_zones_bit_for_bit():
    node_off, row, slot, node, e, p = run(bits(np.nan))
    assert slot.tolist() == [5, 2, 7, 0, 1, 3, 4, 6]  # the NEW bit is masked off
    assert node.tolist() == [0, 0, 0, 1, 1, 3, 3, 3]
    assert e.tolist() == [[500, 501], [200, 201], [700, 701], [0, 1], [100, 101], [300, 301], [400, 401], [600, 601]]
    assert p.dtype == np.uint64 and p.shape == (8, 2)
    assert p[:, 0].view(np.float64).tolist() == [50.0, 20.0, 70.0, 0.0, 10.0, 30.0, 40.0, 60.0]
    assert p[:, 1].tolist() == [bits(1.5), 0, bits(3.0), bits(np.nan), 1 << 63, bits(-2.5), bits(np.inf), 1]
    assert [a.dtype for a in (node_off, row, slot, node, e)] == [np.uint32] * 4 + [np.uint64]


def test_energy_thresholds():
    assert rows_and_off(run(0, by_power=False, zone=0)) == ([0, 1, 2, 3, 4, 5, 6, 7], [0, 3, 5, 5, 8])
    # 300 is slot 3's energy (row 5): kept; zone 1 holds 301 there: not kept at 302
    assert rows_and_off(run(300, by_power=False, zone=0)) == ([0, 2, 5, 6, 7], [0, 2, 2, 2, 5])
    assert rows_and_off(run(302, by_power=False, zone=1)) == ([0, 2, 6, 7], [0, 2, 2, 2, 4])
    out = run(702, by_power=False, zone=1)  # above the largest
    assert rows_and_off(out) == ([], [0, 0, 0, 0, 0])
    assert out[4].shape == (0, 2) and out[5].shape == (0, 2)


def test_masked_and_read_error_nodes_contribute_nothing():
    assert rows_and_off(run(bits(np.nan), mask=[1, 0, 1, 7])) == ([0, 1, 2, 5, 6, 7], [0, 3, 3, 3, 6])
    assert rows_and_off(run(bits(np.nan), status=[0, 0, 0, 1])) == ([0, 1, 2, 3, 4], [0, 3, 5, 5, 5])
    # status bits other than the read error do not unlist; both together
    assert rows_and_off(run(bits(np.nan), status=[2, 1, 0, 0], mask=[1, 1, 1, 0])) == ([0, 1, 2], [0, 3, 3, 3, 3])


def test_cap_below_at_and_above_the_total():
    full = run(bits(0.0))  # six items
    for cap, k in ((0, 0), (5, 5), (6, 6), (9, 6)):
        out = run(bits(0.0), cap=cap)
        assert out[0].tolist() == [0, 3, 4, 4, 6]  # always the full offsets
        assert out[1].tolist() == [0, 1, 2, 4, 6, 7][:k]
        for got, want in zip(out[1:], full[1:]):
            assert got.shape[0] == k
            np.testing.assert_array_equal(got, want[:k])
