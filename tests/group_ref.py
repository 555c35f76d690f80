"""The contract of kacc_group_sums (include/kepler_accel.h), restated in numpy.

Fed like tests/select_ref.py: the kind's state tables in the logical [slot * Z + zone] layout (the
oracle's ``ora.state[...]`` or ``Accel.download``) and the batch's offsets, slot words, node status,
node mask and group ids; returns the five outputs of one call.
"""

import numpy as np

from top_ref import KACC_NODE_READ_ERROR, KACC_SLOT_MASK

KACC_GROUP_NONE = 0xFFFFFFFF
KACC_GROUP_MAX = 65536
FRAC_BITS = 12
LIMIT = 2.0 ** 50  # |p| at or past it is dropped


def fx(p):
    """(fx words u64, dropped bool) of an f64 array: trunc(p * 4096) as a two's-complement i64 for a
    finite |p| < 2^50, else 0 and dropped."""
    p = np.asarray(p, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        keep = np.isfinite(p) & (np.abs(p) < LIMIT)
    scaled = np.where(keep, p, 0.0) * float(1 << FRAC_BITS)  # exact: a power of two, |.| < 2^62
    return np.trunc(scaled).astype(np.int64).view(np.uint64), ~keep


def power_of(power_fx):
    """out_power of out_power_fx: the i64 correctly rounded to f64 (numpy's int64 -> float64 is the
    C conversion, nearest even), scaled exactly."""
    return np.asarray(power_fx, dtype=np.uint64).view(np.int64).astype(np.float64) * 2.0 ** -FRAC_BITS


def contributing(row_off, slot_words, node_status, node_mask, group, n_groups, capacity=None):
    """Bool [n_rows]: the rows that contribute (listed node, group id below n_groups, slot below the
    capacity when one is given)."""
    row_off = np.asarray(row_off, dtype=np.int64)
    n_nodes = len(row_off) - 1
    status = np.zeros(n_nodes, dtype=np.uint32) if node_status is None else np.asarray(node_status, dtype=np.uint32)
    listed = (status & np.uint32(KACC_NODE_READ_ERROR)) == 0
    if node_mask is not None:
        listed &= np.asarray(node_mask) != 0
    node_of_row = np.repeat(np.arange(n_nodes), np.diff(row_off))
    ok = listed[node_of_row] & (np.asarray(group, dtype=np.uint32) < np.uint32(min(n_groups, 2**32 - 1)))
    if capacity is not None:
        ok &= (np.asarray(slot_words, dtype=np.uint32) & np.uint32(KACC_SLOT_MASK)).astype(np.int64) < capacity
    return ok


def group_sums(energy, power, zones, row_off, slot_words, node_status, node_mask, group, n_groups):
    """Expected outputs of one call.

    energy (u64) and power (f64) are the kind's tables [S * zones]; row_off [N + 1], slot_words
    [n_rows], node_status ([N] or None) are the batch's; node_mask is [N] (nonzero = listed) or None;
    group is u32 [n_rows].  A row whose slot is past the tables is left out (the call also raises
    KACC_ERANGE for it, as for an id >= n_groups other than KACC_GROUP_NONE).  Returns (count u32
    [G], energy u64 [G, Z], power_fx u64 [G, Z], power f64 [G, Z], dropped u32 [G])."""
    e = np.ascontiguousarray(np.asarray(energy, dtype=np.uint64).reshape(-1, zones))
    p = np.ascontiguousarray(np.asarray(power, dtype=np.float64).reshape(-1, zones))
    ok = contributing(row_off, slot_words, node_status, node_mask, group, n_groups, capacity=e.shape[0])
    rows = np.flatnonzero(ok)
    s = (np.asarray(slot_words, dtype=np.uint32)[rows] & np.uint32(KACC_SLOT_MASK)).astype(np.int64)
    g = np.asarray(group, dtype=np.uint32)[rows].astype(np.int64)
    words, drop = fx(p[s])
    count = np.bincount(g, minlength=n_groups).astype(np.uint32)
    dropped = np.zeros(n_groups, dtype=np.int64)
    np.add.at(dropped, g, drop.sum(axis=1))
    out_e = np.zeros((n_groups, zones), dtype=np.uint64)
    out_fx = np.zeros((n_groups, zones), dtype=np.uint64)
    with np.errstate(over="ignore"):
        np.add.at(out_e, g, e[s])  # u64 adds wrap: the sums are mod 2^64
        np.add.at(out_fx, g, words)
    return count, out_e, out_fx, power_of(out_fx), dropped.astype(np.uint32)
