"""tests/gtop_ref.py against a brute-force restatement in plain Python (a sorted list per group on
Python ints), against tests/top_ref.py for the two identities of the header, and on the rules a
vectorised restatement gets wrong most easily: the tie cut, the NaN rank, the zeros' bits."""

import struct

import numpy as np
import pytest

from group_ref import KACC_GROUP_NONE
from gtop_ref import group_top, merge_shards
from top_ref import KACC_NODE_READ_ERROR, top_lists

MASK64 = (1 << 64) - 1
FILL = 0xFFFFFFFF


def bits_of(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def py_key(bits, is_power):
    """The header's key of one value, on Python ints: a NaN power is 0."""
    if not is_power:
        return bits
    mag = bits & (MASK64 >> 1)
    if mag > 0x7FF0000000000000:
        return 0
    if mag == 0:
        return 1 << 63
    return (~bits & MASK64) if bits >> 63 else bits | 1 << 63


def brute(bits, is_power, zones, zone, row_off, words, status, mask, group, n_groups, k):
    """The five outputs as nested Python lists."""
    cap = len(bits) // zones
    lists = [[] for _ in range(n_groups)]
    for n in range(len(row_off) - 1):
        if status is not None and int(status[n]) & KACC_NODE_READ_ERROR:
            continue
        if mask is not None and int(mask[n]) == 0:
            continue
        for r in range(int(row_off[n]), int(row_off[n + 1])):
            s = int(words[r]) & 0x7FFFFFFF
            g = 0 if group is None else int(group[r])
            if s >= cap or g >= n_groups:
                continue
            b = int(bits[s * zones + zone])
            lists[g].append((-py_key(b, is_power), r, s, n, b))
    count, row, slot, node, value = [], [], [], [], []
    for g in range(n_groups):
        best = sorted(lists[g])[:k]  # descending key, then ascending row: the tuple's order
        pad = k - len(best)
        count.append(len(best))
        row.append([e[1] for e in best] + [FILL] * pad)
        slot.append([e[2] for e in best] + [FILL] * pad)
        node.append([e[3] for e in best] + [FILL] * pad)
        value.append([e[4] for e in best] + [0] * pad)
    return count, row, slot, node, value


def random_case(seed, is_power):
    rng = np.random.default_rng(seed)
    zones = int(rng.integers(1, 5))
    zone = int(rng.integers(0, zones))
    sizes = rng.integers(0, 40, int(rng.integers(1, 9)))
    row_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    n_rows, n_nodes = int(row_off[-1]), sizes.size
    cap = n_rows + 5
    words = rng.permutation(cap)[:n_rows].astype(np.uint32)
    words[rng.random(n_rows) < 0.3] |= np.uint32(0x80000000)  # KACC_SLOT_NEW is ignored
    if n_rows:
        words[int(rng.integers(0, n_rows))] = np.uint32(cap + 3)  # a slot past the capacity
    if is_power:
        pool = np.array([0.0, -0.0, 1.5, 1.5, -2.0, np.inf, -np.inf, np.nan, 3.25, 1e-300, 7.0, 7.0])
        table = rng.choice(pool, cap * zones)
        bits = np.ascontiguousarray(table).view(np.uint64)
    else:
        table = rng.choice(np.array([0, 1, 5, 5, 5, 2 ** 63, 2 ** 64 - 1, 77, 1 << 40], dtype=np.uint64), cap * zones)
        bits = table
    n_groups = int(rng.integers(1, 12)) + 2  # the last two groups stay empty
    group = rng.integers(0, n_groups - 2, n_rows).astype(np.uint32)
    group[rng.random(n_rows) < 0.1] = KACC_GROUP_NONE
    status = (rng.random(n_nodes) < 0.2).astype(np.uint32) * np.uint32(KACC_NODE_READ_ERROR)
    mask = (rng.random(n_nodes) < 0.7).astype(np.uint32) * np.uint32(5)
    return dict(table=table, bits=bits, zones=zones, zone=zone, row_off=row_off, words=words, status=status, mask=mask,
                group=group, n_groups=n_groups)


@pytest.mark.parametrize("is_power", [False, True])
@pytest.mark.parametrize("seed", range(12))
def test_reference_equals_a_plain_loop(seed, is_power):
    c = random_case(seed, is_power)
    biggest = 0
    for k in (1, 3, 400):  # 400: more than the batch has rows
        for group, n_groups, mask in ((c["group"], c["n_groups"], c["mask"]), (c["group"], c["n_groups"], None),
                                      (None, 1, c["mask"])):
            got = group_top(c["table"], is_power, c["zones"], c["zone"], c["row_off"], c["words"], c["status"], mask,
                            group, n_groups, k)
            want = brute(c["bits"], is_power, c["zones"], c["zone"], c["row_off"], c["words"], c["status"], mask, group,
                         n_groups, k)
            assert got[0].dtype == np.uint32 and got[4].dtype == np.uint64 and got[1].shape == (n_groups, k)
            for g_arr, w in zip(got, want):
                assert g_arr.tolist() == w
            if group is not None:
                assert got[0][-2:].tolist() == [0, 0] and (got[1][-2:] == FILL).all() and not got[4][-2:].any()
            biggest = max(biggest, int(got[0].max()))
    assert 0 < biggest < 400  # k was greater than a group's rows


@pytest.mark.parametrize("is_power", [False, True])
def test_the_two_identities_with_the_top_lists(is_power):
    c = random_case(40, is_power)
    n_nodes = c["row_off"].size - 1
    node_ids = np.repeat(np.arange(n_nodes), np.diff(c["row_off"].astype(np.int64))).astype(np.uint32)
    # top_ref has no capacity check: keep every slot inside the table
    words = c["words"].copy()
    words[(words & np.uint32(0x7FFFFFFF)) >= c["table"].size // c["zones"]] = 0
    for k in (1, 4, 64):
        top = top_lists(c["table"], c["zones"], c["zone"], is_power, c["row_off"], words, c["status"], k)
        fleet = group_top(c["table"], is_power, c["zones"], c["zone"], c["row_off"], words, c["status"], None, None, 1, k)
        for got, want in zip(fleet, top["fleet"]):
            np.testing.assert_array_equal(got.reshape(-1), want.reshape(-1))
        count, row, slot, _, value = group_top(c["table"], is_power, c["zones"], c["zone"], c["row_off"], words,
                                               c["status"], None, node_ids, n_nodes, k)
        for got, want in zip((count, row, slot, value), top["nodes"]):
            np.testing.assert_array_equal(got, want)


def one_node(values, is_power, group, n_groups, k):
    v = np.asarray(values, dtype=np.float64 if is_power else np.uint64)
    return group_top(v, is_power, 1, 0, [0, v.size], np.arange(v.size, dtype=np.uint32), None, None, group, n_groups, k)


def test_equal_keys_keep_the_lowest_rows():
    group = np.array([0, 1, 0, 1, 0, 1, 0, 1, 0], dtype=np.uint32)
    count, row, _, _, value = one_node([9] * 9, False, group, 2, 3)
    assert count.tolist() == [3, 3] and row.tolist() == [[0, 2, 4], [1, 3, 5]] and (value == 9).all()
    # two values: the cut inside the tie block (group 0) and on its edge (group 1)
    count, row, _, _, _ = one_node([5, 9, 9, 9, 5, 9, 5, 5, 5], False, group, 2, 3)
    assert row.tolist() == [[2, 0, 4], [1, 3, 5]]


def test_nan_is_ranked_last_in_row_order_and_keeps_its_bits():
    nan_a, nan_b = 0x7FF8000000000123, 0xFFF0000000000001
    bits = np.array([nan_a, bits_of(-np.inf), nan_b, bits_of(1.0), nan_a], dtype=np.uint64)
    count, row, _, _, value = one_node(bits.view(np.float64), True, None, 1, 5)
    assert count.tolist() == [5] and row.tolist() == [[3, 1, 0, 2, 4]]
    assert value[0].tolist() == [bits_of(1.0), bits_of(-np.inf), nan_a, nan_b, nan_a]


def test_the_zeros_share_a_key_and_keep_their_bits():
    count, row, _, _, value = one_node([-0.0, 0.0, -1.0, -0.0, 0.0], True, None, 1, 4)
    assert row.tolist() == [[0, 1, 3, 4]]
    assert value[0].tolist() == [bits_of(-0.0), 0, bits_of(-0.0), 0]


def test_shards_merge_to_the_whole():
    c = random_case(41, True)
    n_nodes = c["row_off"].size - 1
    half = (np.arange(n_nodes) % 2).astype(np.uint32)
    args = (c["table"], True, c["zones"], c["zone"], c["row_off"], c["words"], c["status"])
    for k in (1, 5):
        whole = group_top(*args, None, c["group"], c["n_groups"], k)
        parts = [group_top(*args, m, c["group"], c["n_groups"], k) for m in (half, 1 - half)]
        for got, want in zip(merge_shards(parts, True, k), whole):
            np.testing.assert_array_equal(got, want)
