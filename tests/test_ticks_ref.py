"""tests/ticks_ref.py pinned on values worked out by hand (no GPU), and accel.encode_ticks decoded by
it: the increments at the 16-bit boundary, negative and 2^63 increments, now < prev, NEW rows."""

import numpy as np

from kepler_amd import accel
from ticks_ref import ESCAPED, READ_ERROR, SLOT_NEW, TicksRef, cpu_delta, cpu_time


def test_float64_of_uint64_rounds_to_nearest_even():
    # 53 significand bits: above 2^53 the spacing is 2, a tie goes to the even significand
    assert float(2**53 + 1) == 2.0**53                 # tie between 2^53 and 2^53+2: 2^53 is even
    assert float(2**53 + 3) == 2.0**53 + 4             # tie between +2 (odd) and +4 (even)
    assert float(2**64 - 1) == 2.0**64                 # spacing 2048 below 2^64: rounds up
    assert cpu_time(2**53 + 1) == 2.0**53 / 100.0
    assert cpu_time(2**64 - 1) == 2.0**64 / 100.0
    assert cpu_time(250) == 2.5 and cpu_time(1) == 0.01


def test_one_tick_after_two_to_the_53_is_no_time():
    assert cpu_delta(2**53, 2**53 + 1) == 0.0
    assert cpu_delta(2**53, 2**53 + 2) == (2.0**53 + 2) / 100.0 - 2.0**53 / 100.0
    assert cpu_delta(0, 7) == 0.07
    assert cpu_delta(100, 350) == 2.5
    assert cpu_delta(300, 100) == -2.0                 # a reused PID: the ticks went back


def test_division_is_not_a_reciprocal_multiply():
    bad = [v for v in range(1, 20000) if float(v) / 100.0 != float(v) * 0.01]
    assert len(bad) == 2661 and bad[:4] == [35, 41, 47, 57]
    assert cpu_time(35) == 0.35 and 35 * 0.01 == 0.35000000000000003


def test_rows_new_wrap_and_skip_by_hand():
    ref = TicksRef(4)
    d, err = ref.delta(1, [0, 3], [SLOT_NEW | 2, SLOT_NEW | 0, SLOT_NEW | 3], [250, ESCAPED, 0], [0, 1], [1], [-1])
    assert not err and d == [2.5, 2.0**64 / 100.0, 0.0] and ref.map == [2**64 - 1, 0, 250, 0]
    # slot 0 wraps to 0: Δ = 0/100 - 2^64/100; slot 2: 250 -> 300; slot 3 NEW again on a zero entry
    d, err = ref.delta(1, [0, 3], [2, 0, SLOT_NEW | 3], [50, 1, 9])
    assert not err and d == [0.5, -(2.0**64) / 100.0, 0.09] and ref.map == [0, 0, 300, 9]
    # a NEW row of a used slot starts from 0, in the regular and in the escape path
    d, err = ref.delta(1, [0, 2], [SLOT_NEW | 2, SLOT_NEW | 3], [100, ESCAPED], [0, 1], [1], [70000])
    assert not err and d == [1.0, 700.0] and ref.map == [0, 0, 100, 70000]
    # a READ_ERROR node: rows not written, map not moved
    d, err = ref.delta(2, [0, 1, 2], [2, 3], [5, 5], node_status=[READ_ERROR, 0])
    assert not err and d == [None, 700.05 - 700.0] and ref.map == [0, 0, 100, 70005]


def test_documented_errors_by_hand():
    ref = TicksRef(2)
    d, err = ref.delta(1, [0, 2], [SLOT_NEW | 5, SLOT_NEW | 1], [3, 4])          # a slot past the capacity
    assert err and d == [0.0, 0.04] and ref.map == [0, 4]
    d, err = ref.delta(1, [0, 2], [0, 1], [ESCAPED, 1])                            # an escaped row, no escape
    assert err and d == [0.0, 0.05 - 0.04] and ref.map == [0, 5]
    d, err = ref.delta(2, [0, 1, 2], [0, 1], [ESCAPED, 1], [0, 0, 1], [0], [9])  # the escape in another node
    assert err and d == [0.0, 0.06 - 0.05] and ref.map == [0, 6]
    d, err = ref.delta(1, [0, 2], [0, 1], [ESCAPED, ESCAPED], [0, 2], [1, 1], [9, 9])  # the same row twice
    assert err and d == [0.0, 0.15 - 0.06] and ref.map == [0, 15]
    d, err = ref.delta(1, [0, 3], [0, 1], [1, 1])                                  # proc_off past n_procs
    assert err and d == [0.01, 0.16 - 0.15] and ref.map == [1, 16]


def test_encode_ticks_decodes_to_the_readings():
    M = 1 << 64
    incs = [0, 0xFFFE, 0xFFFF, 0x10000, -1, 2**63]
    prev = [10**6 + i for i in range(len(incs))] + [5000, 123456]
    now = [(p + i) % M for p, i in zip(prev, incs)] + [1200, 2**40]  # now < prev; a NEW row's first reading
    new = [False] * (len(incs) + 1) + [True]
    # nodes: empty, rows 0..2, empty, rows 3..7, empty
    proc_off = np.array([0, 0, 3, 3, 8, 8], dtype=np.uint32)
    base = [0 if nw else p for p, nw in zip(prev, new)]
    dt, esc_off, esc_row, esc_ticks = accel.encode_ticks(proc_off, np.array(now, np.uint64), np.array(base, np.uint64))
    assert dt.tolist() == [0, 0xFFFE, ESCAPED, ESCAPED, ESCAPED, ESCAPED, ESCAPED, ESCAPED]
    assert esc_row.tolist() == [2, 3, 4, 5, 6, 7] and esc_off.tolist() == [0, 0, 1, 1, 6, 6]
    assert esc_ticks.tolist() == [0xFFFF, 0x10000, -1, -2**63, 1200 - 5000, 2**40]
    for n in range(5):
        r = esc_row[esc_off[n]:esc_off[n + 1]].astype(np.int64)
        assert (np.diff(r) > 0).all() and ((r >= proc_off[n]) & (r < proc_off[n + 1])).all()
    ref = TicksRef(8)
    ref.map = list(prev)
    words = [i | (SLOT_NEW if nw else 0) for i, nw in enumerate(new)]
    d, err = ref.delta(5, proc_off, words, dt, esc_off, esc_row, esc_ticks)
    assert not err and ref.map == now
    assert d == [cpu_delta(b, w) for b, w in zip(base, now)]
