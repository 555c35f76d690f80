"""The rule of kacc_select_above (include/kepler_accel.h), restated in numpy on top_ref.sort_key.

Fed from state tables in the logical [slot * Z + zone] layout (the oracle's ``ora.state[...]`` or
``Accel.download``) and the batch's offsets, slot words and node status; returns the expected
per-node offsets and the items an output of ``item_cap`` items holds.
"""

import numpy as np

from top_ref import KACC_NODE_READ_ERROR, KACC_SLOT_MASK, sort_key


def threshold_key(threshold_bits, by_power):
    """The u64 key of the threshold: µJ, or the bits of the f64 µW under the powers' rule."""
    bits = np.array([threshold_bits], dtype=np.uint64)
    return sort_key(bits.view(np.float64) if by_power else bits, by_power)[0]


def select_above(energy, power, zones, zone, by_power, row_off, slot_words, node_status, node_mask,
                 threshold_bits, item_cap):
    """Expected outputs of one call.

    energy (u64) and power (f64) are the kind's tables [S * zones]; the predicate reads ``power``
    when by_power, else ``energy``, in ``zone``.  row_off [N + 1], slot_words [n_rows], node_status
    ([N] or None) are the batch's; node_mask is [N] (nonzero = listed) or None.  Returns
    (node_off u32 [N + 1] — always the full offsets —, row u32 [k], slot u32 [k], node u32 [k],
    energy u64 [k, zones], power BITS u64 [k, zones]) with k = min(total, item_cap)."""
    row_off = np.asarray(row_off, dtype=np.int64)
    n_nodes = len(row_off) - 1
    slots = (np.asarray(slot_words, dtype=np.uint32) & np.uint32(KACC_SLOT_MASK)).astype(np.int64)
    e = np.ascontiguousarray(np.asarray(energy, dtype=np.uint64).reshape(-1, zones))
    p = np.ascontiguousarray(np.asarray(power, dtype=np.float64).reshape(-1, zones))
    vals = np.ascontiguousarray((p if by_power else e)[slots, zone])
    key = sort_key(vals, by_power)
    status = np.zeros(n_nodes, dtype=np.uint32) if node_status is None else np.asarray(node_status, dtype=np.uint32)
    listed = (status & np.uint32(KACC_NODE_READ_ERROR)) == 0
    if node_mask is not None:
        listed &= np.asarray(node_mask) != 0
    node_of_row = np.repeat(np.arange(n_nodes), np.diff(row_off))
    selected = listed[node_of_row] & (key >= threshold_key(threshold_bits, by_power))
    before = np.r_[0, np.cumsum(selected)]  # selected rows in front of row r
    node_off = before[row_off].astype(np.uint32)
    rows = np.flatnonzero(selected)[:item_cap]
    s = slots[rows]
    return (node_off, rows.astype(np.uint32), s.astype(np.uint32), node_of_row[rows].astype(np.uint32),
            e[s].reshape(-1, zones), p.view(np.uint64)[s].reshape(-1, zones))
