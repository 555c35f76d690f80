"""The contract of kacc_group_top (include/kepler_accel.h), restated in numpy.

Fed like tests/quant_ref.py: the table in the logical [slot * Z + zone] layout (the oracle's
``ora.state[...]`` or ``Accel.download``), the batch's offsets, slot words, node status, node mask
and group ids (None: every row in group 0); returns the five outputs of one call, the 0xffffffff /
0 fill past the count included.  The order is tests/top_ref.py's: descending sort key, equal keys in
ascending batch row order; a NaN power (key 0) is ranked last, not dropped.
"""

import numpy as np

from group_ref import contributing
from top_ref import FILL, KACC_SLOT_MASK, sort_key

KACC_TOP_MAX = 1024
KACC_GROUP_TOP_MAX_ITEMS = 1 << 20


def group_top(table, is_power, zones, zone, row_off, slot_words, node_status, node_mask, group, n_groups, k):
    """Expected outputs of one call.

    table is the state table [S * zones] (u64 energies or f64 powers).  A row whose slot is past the
    table is left out (the call also raises KACC_ERANGE for it, as for an id >= n_groups other than
    KACC_GROUP_NONE).  Returns (count u32 [G], row u32 [G, k], slot u32 [G, k], node u32 [G, k],
    value u64 [G, k]): values are µJ, or the table's own bits of the f64 µW."""
    assert 1 <= k <= KACC_TOP_MAX and n_groups * k <= KACC_GROUP_TOP_MAX_ITEMS
    dt = np.float64 if is_power else np.uint64
    tab = np.ascontiguousarray(np.asarray(table, dtype=dt).reshape(-1, zones))
    words = np.asarray(slot_words, dtype=np.uint32)
    row_off = np.asarray(row_off, dtype=np.int64)
    if group is None:
        assert n_groups == 1
        group = np.zeros(words.size, dtype=np.uint32)
    ok = contributing(row_off, words, node_status, node_mask, group, n_groups, capacity=tab.shape[0])
    rows = np.flatnonzero(ok)
    s = (words[rows] & np.uint32(KACC_SLOT_MASK)).astype(np.int64)
    g = np.asarray(group, dtype=np.uint32)[rows].astype(np.int64)
    vals = np.ascontiguousarray(tab[s, zone])
    bits = vals.view(np.uint64)
    key = sort_key(vals, is_power)
    node_of_row = np.repeat(np.arange(len(row_off) - 1), np.diff(row_off))

    order = np.lexsort((rows, ~key, g))  # by group, then descending key, then ascending row
    g_sorted = g[order]
    n = np.bincount(g, minlength=n_groups).astype(np.int64)
    start = np.cumsum(n) - n
    place = np.arange(order.size) - start[g_sorted]  # the position inside the group's ranking
    keep = place < k
    at_g, at_i, src = g_sorted[keep], place[keep], order[keep]

    out_row = np.full((n_groups, k), FILL, dtype=np.uint32)
    out_slot = np.full((n_groups, k), FILL, dtype=np.uint32)
    out_node = np.full((n_groups, k), FILL, dtype=np.uint32)
    out_value = np.zeros((n_groups, k), dtype=np.uint64)
    out_row[at_g, at_i] = rows[src]
    out_slot[at_g, at_i] = s[src]
    out_node[at_g, at_i] = node_of_row[rows[src]]
    out_value[at_g, at_i] = bits[src]
    return np.minimum(n, k).astype(np.uint32), out_row, out_slot, out_node, out_value


def merge_shards(shards, is_power, k):
    """The header's cluster rule for shards of ONE batch (global row indices, so "shard order, row
    ascending" is row ascending): the shards' lists of a group merged by (key descending, row
    ascending) and cut to k.  shards: a list of the five outputs."""
    G = shards[0][0].size
    out = (np.zeros(G, dtype=np.uint32), *(np.full((G, k), FILL, dtype=np.uint32) for _ in range(3)),
           np.zeros((G, k), dtype=np.uint64))
    for g in range(G):
        row = np.concatenate([s[1][g, :s[0][g]] for s in shards])
        slot = np.concatenate([s[2][g, :s[0][g]] for s in shards])
        node = np.concatenate([s[3][g, :s[0][g]] for s in shards])
        value = np.concatenate([s[4][g, :s[0][g]] for s in shards])
        key = sort_key(value.view(np.float64) if is_power else value, is_power)
        order = np.lexsort((row, ~key))[:k]
        c = order.size
        out[0][g] = c
        out[1][g, :c], out[2][g, :c], out[3][g, :c], out[4][g, :c] = row[order], slot[order], node[order], value[order]
    return out
