"""tests/group_ref.py (the contract of kacc_group_sums in numpy) against values written out here,
and the two properties the fixed-point sums exist for: the order of the rows and a split of the
rows into shards change no output word.
"""

import numpy as np

from group_ref import KACC_GROUP_NONE, contributing, fx, group_sums, power_of

Z = 2
ROW_OFF = [0, 3, 5, 5, 8]
NEW = 0x80000000  # KACC_SLOT_NEW: ignored
SLOT_WORDS = np.array([5, 2 | NEW, 7, 0, 1, 3, 4, 6], dtype=np.uint32)
#                 slot 0     1     2    3     4       5     6        7
P1 = np.array([np.nan, -0.0, 0.25, -2.5, np.inf, 1.5, 2.0 ** 50, 3.0])
POWER = np.stack([np.arange(8) * 10.0, P1], axis=1).reshape(-1)
ENERGY = np.array([[100 * s, 100 * s + 1] for s in range(8)], dtype=np.uint64).reshape(-1)
GROUP = np.array([0, 1, 0, 1, KACC_GROUP_NONE, 2, 0, 1], dtype=np.uint32)
# rows: slot 5 g0, slot 2 g1, slot 7 g0 | slot 0 g1, slot 1 none | | slot 3 g2, slot 4 g0, slot 6 g1
M64 = 2**64


def run(status=None, mask=None, group=GROUP, n_groups=3):
    return group_sums(ENERGY, POWER, Z, ROW_OFF, SLOT_WORDS, status, mask, group, n_groups)


def test_fx_known_answers():
    below = np.nextafter(2.0 ** 50, 0.0)
    p = np.array([0.5, -0.5, 2.0 ** -13, -0.0, np.nan, np.inf, -np.inf, 2.0 ** 50, -(2.0 ** 50), below, -below,
                  1.0 + 2.0 ** -12 + 2.0 ** -13, -(1.0 + 2.0 ** -12 + 2.0 ** -13), 1e300, 5e-324])
    words, dropped = fx(p)
    assert words.dtype == np.uint64
    want = [2048, M64 - 2048, 0, 0, 0, 0, 0, 0, 0, 2**62 - 2**9, M64 - (2**62 - 2**9), 4097, M64 - 4097, 0, 0]
    assert [int(w) for w in words] == want
    assert dropped.tolist() == [False] * 4 + [True] * 5 + [False] * 4 + [True, False]
    # just below 2^50 is kept exactly: 53 significant bits, 12 of them after the binary point
    assert int(words[9]) == int(below * 4096.0)
    assert power_of(words[:2]).tolist() == [0.5, -0.5]


def test_power_of_rounds_to_nearest_even():
    # 2^53 + 1 and 2^53 + 3 lie halfway between doubles: to the even neighbour
    w = np.array([2**53 + 1, 2**53 + 3, M64 - (2**53 + 1), 2**62], dtype=np.uint64)
    assert power_of(w).tolist() == [2.0 ** 41, (2**53 + 4) / 4096.0, -(2.0 ** 41), 2.0 ** 50]


def test_sums_of_the_small_batch():
    count, e, pfx, p, dropped = run()
    assert count.tolist() == [3, 3, 1]
    # g0: slots 5, 7, 4;  g1: slots 2, 0, 6;  g2: slot 3
    assert e.tolist() == [[500 + 700 + 400, 501 + 701 + 401], [200 + 0 + 600, 201 + 1 + 601], [300, 301]]
    assert pfx[:, 0].tolist() == [(50 + 70 + 40) * 4096, (20 + 0 + 60) * 4096, 30 * 4096]
    # zone 1: g0 = 1.5 + 3.0 + (Inf dropped); g1 = 0.25 + (NaN dropped) + (2^50 dropped); g2 = -2.5
    assert pfx[:, 1].tolist() == [int(4.5 * 4096), 1024, M64 - int(2.5 * 4096)]
    assert p[:, 1].tolist() == [4.5, 0.25, -2.5]
    assert dropped.tolist() == [1, 2, 0]
    assert [a.dtype for a in (count, e, pfx, p, dropped)] == [np.uint32, np.uint64, np.uint64, np.float64, np.uint32]


def test_unlisted_nodes_and_ids_out_of_range_contribute_nothing():
    count = run(mask=[1, 0, 1, 7])[0]
    assert count.tolist() == [3, 2, 1]
    count = run(status=[0, 0, 0, 1])[0]  # node 3: rows 5, 6, 7
    assert count.tolist() == [2, 2, 0]
    count, e = run(status=[2, 1, 0, 0], mask=[1, 1, 1, 0])[:2]  # other status bits do not unlist
    assert count.tolist() == [2, 1, 0] and e[2].tolist() == [0, 0]
    # n_groups 2: id 2 is out of range and left out like KACC_GROUP_NONE
    count, e = run(n_groups=2)[:2]
    assert count.tolist() == [3, 3] and e.shape == (2, Z)
    assert contributing(ROW_OFF, SLOT_WORDS, None, None, GROUP, 2).tolist() == [1, 1, 1, 1, 0, 0, 1, 1]
    # a slot past the tables is left out
    words = SLOT_WORDS.copy()
    words[0] = 8
    assert group_sums(ENERGY, POWER, Z, ROW_OFF, words, None, None, GROUP, 3)[0].tolist() == [2, 3, 1]


def big_case(seed=5, n_rows=5000, n_groups=37, zones=3):
    rng = np.random.default_rng(seed)
    sizes = rng.multinomial(n_rows, np.ones(9) / 9)
    row_off = np.r_[0, np.cumsum(sizes)]
    slots = rng.permutation(n_rows + 100)[:n_rows].astype(np.uint32)
    energy = rng.integers(0, 2**64, size=(n_rows + 100) * zones, dtype=np.uint64)  # the sums wrap
    power = rng.normal(0, 1e9, size=(n_rows + 100) * zones)
    power[rng.integers(0, power.size, 50)] = [np.nan, np.inf, -np.inf, 2.0 ** 50, 1e300] * 10
    power[rng.integers(0, power.size, 50)] = rng.choice([2.0 ** 49, -(2.0 ** 49)], 50)
    group = rng.integers(0, n_groups, n_rows).astype(np.uint32)
    group[rng.random(n_rows) < 0.05] = KACC_GROUP_NONE
    status = (rng.random(9) < 0.2).astype(np.uint32)
    return energy, power, zones, row_off, slots, status, group, n_groups


def permuted_rows(row_off, slots, group, rng):
    """The same rows in another order inside each node (the nodes keep their ranges)."""
    order = np.concatenate([a + rng.permutation(b - a) for a, b in zip(row_off[:-1], row_off[1:])]).astype(np.int64)
    return slots[order], group[order]


def test_row_order_changes_no_output():
    energy, power, zones, row_off, slots, status, group, G = big_case()
    want = group_sums(energy, power, zones, row_off, slots, status, None, group, G)
    assert want[0].sum() > 3000 and want[4].sum() > 0
    rng = np.random.default_rng(1)
    for _ in range(3):
        s2, g2 = permuted_rows(row_off, slots, group, rng)
        got = group_sums(energy, power, zones, row_off, s2, status, None, g2, G)
        for x, y in zip(got, want):
            np.testing.assert_array_equal(x.view(np.uint64) if x.dtype == np.float64 else x, y.view(np.uint64)
                                          if y.dtype == np.float64 else y)


def test_two_shards_add_to_the_whole():
    """The rows split between two shards (each row's group id kept in one, KACC_GROUP_NONE in the
    other): count, dropped, energy and power_fx add word by word mod 2^64, power is that of the sum."""
    energy, power, zones, row_off, slots, status, group, G = big_case(seed=9)
    whole = group_sums(energy, power, zones, row_off, slots, status, None, group, G)
    half = np.random.default_rng(2).random(group.size) < 0.5
    a = group_sums(energy, power, zones, row_off, slots, status, None, np.where(half, group, KACC_GROUP_NONE), G)
    b = group_sums(energy, power, zones, row_off, slots, status, None, np.where(half, KACC_GROUP_NONE, group), G)
    assert a[0].sum() > 1000 and b[0].sum() > 1000
    with np.errstate(over="ignore"):
        for i in (0, 1, 2, 4):
            np.testing.assert_array_equal(a[i] + b[i], whole[i])
        np.testing.assert_array_equal(power_of(a[2] + b[2]).view(np.uint64), whole[3].view(np.uint64))
