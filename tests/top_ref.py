"""The order rule of kacc_top_nodes / kacc_top_fleet (include/kepler_accel.h), restated in numpy.

Fed from state tables in the logical [slot * Z + zone] layout (the oracle's ``ora.state[...]`` or
``Accel.download``) and the batch's slot words; returns the expected output arrays, the
0xffffffff / 0 fill past the count included.
"""

import numpy as np

KACC_SLOT_MASK = 0x7FFFFFFF
KACC_NODE_READ_ERROR = 0x1
FILL = np.uint32(0xFFFFFFFF)
TOP = np.uint64(1) << np.uint64(63)


def sort_key(values, is_power):
    """The u64 sort key of every value: an energy is its own key; a power maps NaN to 0, both
    zeros to the key of +0.0, a positive p to bits | 1<<63 and a negative p to ~bits."""
    if not is_power:
        return np.ascontiguousarray(values, dtype=np.uint64).copy()
    p = np.ascontiguousarray(values, dtype=np.float64)
    b = p.view(np.uint64)
    key = np.where(p > 0, b | TOP, ~b)  # p < 0: ~b
    key = np.where(p == 0, TOP, key)    # either zero counts as +0.0
    return np.where(np.isnan(p), np.uint64(0), key).astype(np.uint64)


def _first(key, rows, k):
    """The first k of `rows` in descending key, ascending row order."""
    order = np.lexsort((rows, ~key[rows]))
    return rows[order[:k]]


def top_lists(table, zones, zone, is_power, row_off, slot_words, node_status, k):
    """Expected outputs of both calls for one table and zone.

    table: the state table [S * zones] (u64 energies or f64 powers); row_off [N + 1], slot_words
    [n_rows] and node_status ([N] or None): the batch's.  Returns a dict: ``nodes`` = (count [N],
    row [N, k], slot [N, k], value [N, k]) and ``fleet`` = (count [1], row [k], slot [k], node [k],
    value [k]); values are u64 (µJ, or the bits of the f64 µW)."""
    row_off = np.asarray(row_off, dtype=np.int64)
    n_nodes = len(row_off) - 1
    slots = (np.asarray(slot_words, dtype=np.uint32) & np.uint32(KACC_SLOT_MASK)).astype(np.int64)
    dt = np.float64 if is_power else np.uint64
    vals = np.ascontiguousarray(np.asarray(table, dtype=dt).reshape(-1, zones)[slots, zone])
    bits = vals.view(np.uint64)
    key = sort_key(vals, is_power)
    status = np.zeros(n_nodes, dtype=np.uint32) if node_status is None else np.asarray(node_status, dtype=np.uint32)
    listed = (status & np.uint32(KACC_NODE_READ_ERROR)) == 0
    node_of_row = np.repeat(np.arange(n_nodes), np.diff(row_off))

    n_count = np.zeros(n_nodes, dtype=np.uint32)
    n_row = np.full((n_nodes, k), FILL, dtype=np.uint32)
    n_slot = np.full((n_nodes, k), FILL, dtype=np.uint32)
    n_value = np.zeros((n_nodes, k), dtype=np.uint64)
    for n in range(n_nodes):
        if not listed[n]:
            continue  # a read-error node lists nothing
        best = _first(key, np.arange(row_off[n], row_off[n + 1]), k)
        c = len(best)
        n_count[n] = c
        n_row[n, :c] = best
        n_slot[n, :c] = slots[best]
        n_value[n, :c] = bits[best]

    best = _first(key, np.flatnonzero(listed[node_of_row]), k)
    c = len(best)
    f_row = np.full(k, FILL, dtype=np.uint32)
    f_slot = np.full(k, FILL, dtype=np.uint32)
    f_node = np.full(k, FILL, dtype=np.uint32)
    f_value = np.zeros(k, dtype=np.uint64)
    f_row[:c] = best
    f_slot[:c] = slots[best]
    f_node[:c] = node_of_row[best]
    f_value[:c] = bits[best]
    return {"nodes": (n_count, n_row, n_slot, n_value),
            "fleet": (np.array([c], dtype=np.uint32), f_row, f_slot, f_node, f_value)}
