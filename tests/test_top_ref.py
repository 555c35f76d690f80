"""The order rule of the top lists, on the CPU: hand-written cases for tests/top_ref.py (the numpy
restatement the GPU tests compare kacc_top_nodes / kacc_top_fleet against), each checked against
literal expected lists, and the ctypes twin of kacc_top_rows against the header."""

import ctypes
import os
import subprocess

import numpy as np

from kepler_amd import accel
from top_ref import sort_key, top_lists

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 0xFFFFFFFF


def bits(*p):
    return np.array(p, dtype=np.float64).view(np.uint64).tolist()


def one_node(values, is_power, k, slots=None):
    """One node, Z = 1, row r in slot slots[r] (identity by default)."""
    n = len(values)
    slots = np.arange(n, dtype=np.uint32) if slots is None else np.asarray(slots, dtype=np.uint32)
    table = np.zeros(int(slots.max()) + 1 if n else 0, dtype=np.float64 if is_power else np.uint64)
    table[slots] = values
    return top_lists(table, 1, 0, is_power, [0, n], slots, None, k)


def test_sort_key_values():
    nan, inf = float("nan"), float("inf")
    key = sort_key(np.array([nan, -inf, -1.5, -0.0, 0.0, 5e-324, 1.0, inf]), True).tolist()
    assert key[0] == 0
    assert key[3] == key[4] == 1 << 63
    assert key == sorted(key)  # NaN < -Inf < -1.5 < ±0 < denormal < 1 < +Inf
    assert len(set(key)) == 7
    assert key[6] == 0x3FF0000000000000 | 1 << 63
    assert key[2] == 0xFFFFFFFFFFFFFFFF ^ 0xBFF8000000000000
    # a negative NaN is a NaN
    assert sort_key(np.array([0xFFF8000000000001], dtype=np.uint64).view(np.float64), True)[0] == 0
    e = np.array([3, 0, 2**64 - 1], dtype=np.uint64)
    assert sort_key(e, False).tolist() == e.tolist()


def test_nan_below_minus_inf():
    nan, inf = float("nan"), float("inf")
    r = one_node([nan, -inf, 2.0, nan], True, 4)
    count, row, slot, value = r["nodes"]
    assert count.tolist() == [4]
    assert row.tolist() == [[2, 1, 0, 3]]  # the NaNs last, by row
    assert value[0, :2].tolist() == bits(2.0, -inf)
    assert np.isnan(value[0, 2:].view(np.float64)).all()
    assert r["fleet"][1].tolist() == [2, 1, 0, 3]


def test_nan_keeps_its_bits_in_the_value():
    neg, pos = 0xFFF8000000000123, 0x7FF8000000BEEF01  # payloads, one with the sign bit
    values = np.array([neg, 0x3FF0000000000000, pos], dtype=np.uint64).view(np.float64)
    r = one_node(values, True, 3)
    assert r["nodes"][1].tolist() == [[1, 0, 2]]
    assert r["nodes"][3].tolist() == [[0x3FF0000000000000, neg, pos]]
    assert r["fleet"][4].tolist() == [0x3FF0000000000000, neg, pos]


def test_minus_zero_ties_with_plus_zero_by_row():
    r = one_node([-0.0, 0.0, -0.0, 1.0, 0.0], True, 4)
    count, row, slot, value = r["nodes"]
    assert row.tolist() == [[3, 0, 1, 2]]
    assert value.tolist() == [bits(1.0, -0.0, 0.0, -0.0)]  # a -0.0 stays -0.0 in the value


def test_negative_powers_below_zero():
    r = one_node([-1.5, 0.0, -1e300, -5e-324, 3.0], True, 5)
    assert r["nodes"][1].tolist() == [[4, 1, 3, 0, 2]]
    assert r["fleet"][4].tolist() == bits(3.0, 0.0, -5e-324, -1.5, -1e300)


def test_equal_energies_ordered_by_row():
    r = one_node([7, 9, 7, 0, 9, 7], False, 5, slots=[5, 4, 3, 2, 1, 0])
    count, row, slot, value = r["nodes"]
    assert count.tolist() == [5]
    assert row.tolist() == [[1, 4, 0, 2, 5]]
    assert slot.tolist() == [[4, 1, 5, 3, 0]]
    assert value.tolist() == [[9, 9, 7, 7, 7]]


def test_k_larger_than_the_row_count_is_filled():
    r = one_node([1, 3, 2], False, 5)
    count, row, slot, value = r["nodes"]
    assert count.tolist() == [3]
    assert row.tolist() == [[1, 2, 0, F, F]]
    assert slot.tolist() == [[1, 2, 0, F, F]]
    assert value.tolist() == [[3, 2, 1, 0, 0]]
    fc, fr, fs, fn, fv = r["fleet"]
    assert fc.tolist() == [3]
    assert fr.tolist() == [1, 2, 0, F, F]
    assert fn.tolist() == [0, 0, 0, F, F]
    assert fv.tolist() == [3, 2, 1, 0, 0]


def test_read_error_node_lists_nothing_and_slot_new_is_ignored():
    # three nodes of 2, 0 and 3 rows, Z = 2, zone 1; node 2 failed its read
    table = np.array([[0, 10], [0, 50], [0, 30], [0, 99], [0, 98], [0, 20]], dtype=np.uint64).reshape(-1)
    slot_words = np.array([2 | 0x80000000, 0, 3, 4, 5], dtype=np.uint32)
    status = np.array([0, 0, 1], dtype=np.uint32)
    r = top_lists(table, 2, 1, False, [0, 2, 2, 5], slot_words, status, 2)
    count, row, slot, value = r["nodes"]
    assert count.tolist() == [2, 0, 0]
    assert row.tolist() == [[0, 1], [F, F], [F, F]]
    assert slot.tolist() == [[2, 0], [F, F], [F, F]]
    assert value.tolist() == [[30, 10], [0, 0], [0, 0]]
    fc, fr, fs, fn, fv = r["fleet"]
    assert (fc.tolist(), fr.tolist(), fs.tolist(), fn.tolist(), fv.tolist()) == ([2], [0, 1], [2, 0], [0, 0], [30, 10])
    # with every node read, node 2's rows lead the fleet list
    r = top_lists(table, 2, 1, False, [0, 2, 2, 5], slot_words, None, 4)
    assert r["nodes"][0].tolist() == [2, 0, 3]
    assert r["fleet"][1].tolist() == [2, 3, 0, 4]
    assert r["fleet"][3].tolist() == [2, 2, 0, 2]


def test_top_rows_layout_matches_header(tmp_path):
    """kacc_top_rows (ABI 6): the ctypes twin's size and every field offset; KACC_TOP_MAX."""
    c = tmp_path / "tr.c"
    fields = [f for f, _ in accel.KaccTopRows._fields_]
    body = "\n".join(f'printf("%zu\\n", offsetof(kacc_top_rows, {f}));' for f in fields)
    c.write_text(f"""
#include <stddef.h>
#include <stdio.h>
#include "kepler_accel.h"
int main(void) {{
  printf("%zu\\n%u\\n%u\\n", sizeof(kacc_top_rows), KACC_TOP_MAX, KACC_ABI_VERSION);
  {body}
  return 0;
}}""")
    exe = tmp_path / "tr"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    vals = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert vals[0] == ctypes.sizeof(accel.KaccTopRows)
    assert vals[1] == accel.KACC_TOP_MAX == 1024
    assert vals[2] == accel.KACC_ABI_VERSION == 6
    for f, off in zip(fields, vals[3:]):
        assert getattr(accel.KaccTopRows, f).offset == off, f
