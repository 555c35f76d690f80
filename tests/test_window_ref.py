"""tests/window_ref.py (the contract of kacc_window_* in numpy) on a hand-made example.

Two nodes, six process slots (node 0 owns 0..3, node 1 owns 4..5), Z = 2, two groups, three
intervals.  The window is marked after interval 1.  In interval 3 the join (reuse policy) finds
slot 1's workload terminated and hands the slot to a newcomer in the same call, and node 1 fails
its read, with a stale KACC_SLOT_NEW left in its row's slot word.  Every figure below is worked
out by hand.
"""

import numpy as np

from group_ref import group_sums
from window_ref import KACC_GROUP_NONE, KACC_NODE_READ_ERROR, KACC_SLOT_NEW, KACC_WINDOW_ASSIGN_ALL, WindowRef

NEW = KACC_SLOT_NEW
Z, S, G = 2, 6, 2
SLOT_OFF = np.array([0, 4, 6])
ROW_OFF = np.array([0, 2, 3])
OK = np.zeros(2, dtype=np.uint32)


def table(rows):
    e = np.zeros((S, Z), dtype=np.uint64)
    for s, v in rows.items():
        e[s] = v
    return e.reshape(-1)


E0 = table({})
E1 = table({0: [10, 1], 1: [20, 2], 4: [5, 5]})
E2 = table({0: [15, 2], 1: [50, 3], 4: [6, 6]})
E3 = table({0: [17, 2], 1: [4, 4], 4: [6, 6]})  # slot 1: the newcomer, from zero; node 1 skipped
# interval -> (tables before, slot words, node status, group ids, term_slot, term_count, tables after)
STEPS = [
    (E0, [0 | NEW, 1 | NEW, 4 | NEW], OK, [0, 1, 1], np.zeros(6, np.uint32), [0, 0], E1),
    (E1, [0, 1, 4], OK, [0, 1, 1], np.zeros(6, np.uint32), [0, 0], E2),
    (E2, [0, 1 | NEW, 4 | NEW], np.array([0, KACC_NODE_READ_ERROR], np.uint32), [0, 0, 0],
     np.array([1, 0, 0, 0, 0, 0], np.uint32), [1, 0], E3),
]


def run(w, upto, mark_after=(), flags=0):
    for i, (before, words, status, group, ts, tc, after) in enumerate(STEPS[:upto]):
        w.step(before, ROW_OFF, np.array(words, np.uint32), status, np.array(group, np.uint32), flags, SLOT_OFF, ts, tc)
        if i in mark_after:
            w.mark(after)
    return STEPS[upto - 1]


def test_a_fresh_window_and_the_first_interval():
    w = WindowRef(S, Z, G)
    assert not w.base.any() and np.all(w.slot_group == KACC_GROUP_NONE)
    assert not w.retired.any() and not w.retired_count.any()
    _, words, status, _, _, _, after = run(w, 1)
    np.testing.assert_array_equal(w.slot_group, [0, 1, KACC_GROUP_NONE, KACC_GROUP_NONE, 1, KACC_GROUP_NONE])
    count, running, retired, rcount, total, row = w.read(after, ROW_OFF, np.array(words, np.uint32), status)
    np.testing.assert_array_equal(count, [1, 2])
    np.testing.assert_array_equal(running, [[10, 1], [25, 7]])
    np.testing.assert_array_equal(row, [[10, 1], [20, 2], [5, 5]])
    np.testing.assert_array_equal(total, running)
    assert not retired.any() and not rcount.any() and not w.erange


def test_a_read_straight_after_the_mark_is_zero():
    w = WindowRef(S, Z, G)
    _, words, status, _, _, _, after = run(w, 1, mark_after={0})
    count, running, _, _, total, row = w.read(after, ROW_OFF, np.array(words, np.uint32), status)
    np.testing.assert_array_equal(count, [1, 2])  # the groups stay
    assert not running.any() and not row.any() and not total.any()
    np.testing.assert_array_equal(w.base.reshape(-1), E1)


def test_the_marked_window_after_interval_two():
    w = WindowRef(S, Z, G)
    _, words, status, _, _, _, after = run(w, 2, mark_after={0})
    count, running, retired, rcount, total, row = w.read(after, ROW_OFF, np.array(words, np.uint32), status)
    np.testing.assert_array_equal(row, [[5, 1], [30, 1], [1, 1]])
    np.testing.assert_array_equal(running, [[5, 1], [31, 2]])
    np.testing.assert_array_equal(total, running)


def test_a_slot_retired_and_adopted_in_one_step():
    w = WindowRef(S, Z, G)
    _, words, status, _, _, _, after = run(w, 3, mark_after={0})
    assert w.reused == 1  # slot 1
    # (a) before (b): slot 1's old workload (group 1) retires with E2 - base = [50, 3] - [20, 2] ...
    np.testing.assert_array_equal(w.retired, [[0, 0], [30, 1]])
    np.testing.assert_array_equal(w.retired_count, [0, 1])
    # ... then the newcomer takes the slot: group 0, base 0.  Node 1's stale NEW word (slot 4, id 0) is not adopted
    np.testing.assert_array_equal(w.slot_group, [0, 0, KACC_GROUP_NONE, KACC_GROUP_NONE, 1, KACC_GROUP_NONE])
    np.testing.assert_array_equal(w.base, [[10, 1], [0, 0], [0, 0], [0, 0], [5, 5], [0, 0]])
    count, running, retired, rcount, total, row = w.read(after, ROW_OFF, np.array(words, np.uint32), status)
    np.testing.assert_array_equal(count, [2, 0])  # node 1 is not listed
    np.testing.assert_array_equal(row, [[7, 1], [4, 4], [0, 0]])
    np.testing.assert_array_equal(running, [[11, 5], [0, 0]])
    np.testing.assert_array_equal(retired, [[0, 0], [30, 1]])
    np.testing.assert_array_equal(rcount, [0, 1])
    np.testing.assert_array_equal(total, [[11, 5], [30, 1]])
    # the same read with node 1 listed: its row's last good totals
    count, running, _, _, total, row = w.read(after, ROW_OFF, np.array(words, np.uint32), None)
    np.testing.assert_array_equal(count, [2, 1])
    np.testing.assert_array_equal(row[2], [1, 1])
    np.testing.assert_array_equal(total, [[11, 5], [31, 2]])
    assert not w.erange


def test_the_total_is_the_sum_of_the_intervals_own_increases():
    whole, each = WindowRef(S, Z, G), WindowRef(S, Z, G)
    acc = np.zeros((G, Z), dtype=np.uint64)
    for i, (before, words, status, group, ts, tc, after) in enumerate(STEPS):
        for w in (whole, each):
            w.step(before, ROW_OFF, np.array(words, np.uint32), status, np.array(group, np.uint32), 0, SLOT_OFF, ts, tc)
        acc += each.read(after, ROW_OFF, np.array(words, np.uint32), None)[4]
        each.mark(after)
    total = whole.read(after, ROW_OFF, np.array(words, np.uint32), None)[4]
    np.testing.assert_array_equal(total, acc)
    np.testing.assert_array_equal(total, [[21, 6], [56, 9]])  # never marked: all the joules, by group
    assert total.sum() == E3.sum() + E2.reshape(S, Z)[1].sum()  # the running totals and the retired workload's


def test_a_mask_and_its_complement_add_up():
    w = WindowRef(S, Z, G)
    _, words, _, _, _, _, after = run(w, 3, mark_after={0})
    words = np.array(words, np.uint32)
    one, other = np.array([1, 0]), np.array([0, 1])
    a, b, both = (w.read(after, ROW_OFF, words, None, m) for m in (one, other, None))
    np.testing.assert_array_equal(a[0] + b[0], both[0])
    np.testing.assert_array_equal(a[1] + b[1], both[1])
    np.testing.assert_array_equal(a[5] + b[5], both[5])
    for r in (a, b):  # the retired part is not masked
        np.testing.assert_array_equal(r[2], both[2])
        np.testing.assert_array_equal(r[3], both[3])
        np.testing.assert_array_equal(r[4], r[1] + r[2])


def test_assign_all_from_the_start_is_the_group_sum():
    w = WindowRef(S, Z, G)
    for i, (before, words, status, group, ts, tc, after) in enumerate(STEPS[:2]):
        words, group = np.array(words, np.uint32), np.array(group, np.uint32)
        w.step(before, ROW_OFF, words, status, group, KACC_WINDOW_ASSIGN_ALL, SLOT_OFF, ts, tc)
        count, running = w.read(after, ROW_OFF, words, status)[:2]
        want = group_sums(after, np.zeros(S * Z), Z, ROW_OFF, words, status, None, group, G)
        np.testing.assert_array_equal(count, want[0])
        np.testing.assert_array_equal(running, want[1])


def test_assign_all_relabels_and_resets_no_running_base():
    w = WindowRef(S, Z, G)
    _, words, status, _, _, _, after = run(w, 2, mark_after={0})
    base = w.base.copy()
    w.step(after, ROW_OFF, np.array(words, np.uint32), status, np.array([1, KACC_GROUP_NONE, 0], np.uint32),
           KACC_WINDOW_ASSIGN_ALL)
    np.testing.assert_array_equal(w.slot_group[[0, 1, 4]], [1, KACC_GROUP_NONE, 0])
    np.testing.assert_array_equal(w.base, base)
    assert not w.erange


def test_the_clamped_cases_are_left_out_and_reported():
    before, words, status, group, ts, tc, after = STEPS[2]
    words, group = np.array(words, np.uint32), np.array(group, np.uint32)
    clean = WindowRef(S, Z, G)
    run(clean, 3, mark_after={0})
    # a terminated slot past the capacity, beside the good one
    w = WindowRef(S, Z, G)
    run(w, 2, mark_after={0})
    w.step(before, ROW_OFF, words, status, group, 0, SLOT_OFF, np.array([1, S, 0, 0, 0, 0], np.uint32), [2, 0])
    assert w.erange
    np.testing.assert_array_equal(w.retired, clean.retired)
    np.testing.assert_array_equal(w.slot_group, clean.slot_group)
    # a count above its segment: the node's list is left out, so nothing retires
    w = WindowRef(S, Z, G)
    run(w, 2, mark_after={0})
    w.step(before, ROW_OFF, words, status, group, 0, SLOT_OFF, ts, [5, 0])
    assert w.erange and not w.retired.any() and not w.retired_count.any()
    # an id of n_groups is stored as no group; a row slot past the capacity is left out
    w = WindowRef(S, Z, G)
    run(w, 2, mark_after={0})
    w.step(before, ROW_OFF, words, status, np.array([0, G, 0], np.uint32), 0, SLOT_OFF, ts, tc)
    assert w.erange and w.slot_group[1] == KACC_GROUP_NONE
    w = WindowRef(S, Z, G)
    run(w, 2, mark_after={0})
    bad = words.copy()
    bad[0] = S
    row = w.read(after, ROW_OFF, bad, status)[5]
    assert w.erange and not row[0].any() and row[1].any()
    # a row range outside the batch: the node's rows are not listed
    w = WindowRef(S, Z, G)
    run(w, 2, mark_after={0})
    count = w.read(after, np.array([0, 2, 4]), words, None)[0]
    assert w.erange
    np.testing.assert_array_equal(count, [1, 1])
