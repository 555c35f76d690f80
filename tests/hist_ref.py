"""The contract of kacc_group_hist (include/kepler_accel.h), restated in numpy.

Fed like tests/group_ref.py: the table in the logical [slot * Z + zone] layout (the oracle's
``ora.state[...]`` or ``Accel.download``), the batch's offsets, slot words, node status, node mask
and group ids (None: every row in group 0) and the bounds as u64 bit patterns; returns the five
outputs of one call.
"""

import numpy as np

from group_ref import contributing, fx
from top_ref import KACC_SLOT_MASK, sort_key

KACC_HIST_MAX_BOUNDS = 64
KACC_HIST_MAX_BINS = 1 << 20


def bound_keys(bounds, is_power):
    """The u64 keys of the bounds (u64 bit patterns: µJ, or the bits of the f64 µW)."""
    b = np.ascontiguousarray(bounds, dtype=np.uint64)
    return sort_key(b.view(np.float64) if is_power else b, is_power)


def bounds_valid(bounds, is_power):
    """The call's rule: 1 .. 64 bounds, keys strictly ascending, no NaN bound for a power table."""
    key = bound_keys(bounds, is_power)
    if not 1 <= key.size <= KACC_HIST_MAX_BOUNDS:
        return False
    if is_power and (key == 0).any():
        return False
    return bool(np.all(key[1:] > key[:-1]))


def group_hist(table, is_power, zones, zone, row_off, slot_words, node_status, node_mask, group, n_groups, bounds):
    """Expected outputs of one call.

    table is the state table [S * zones] (u64 energies or f64 powers).  A row whose slot is past the
    table is left out (the call also raises KACC_ERANGE for it, as for an id >= n_groups other than
    KACC_GROUP_NONE).  Returns (bin u64 [G, B1], cum u64 [G, B1], sum u64 [G], nan u64 [G],
    unsummed u64 [G]) with B1 = len(bounds) + 1."""
    assert bounds_valid(bounds, is_power)
    dt = np.float64 if is_power else np.uint64
    tab = np.ascontiguousarray(np.asarray(table, dtype=dt).reshape(-1, zones))
    words = np.asarray(slot_words, dtype=np.uint32)
    if group is None:
        assert n_groups == 1
        group = np.zeros(words.size, dtype=np.uint32)
    ok = contributing(row_off, words, node_status, node_mask, group, n_groups, capacity=tab.shape[0])
    rows = np.flatnonzero(ok)
    s = (words[rows] & np.uint32(KACC_SLOT_MASK)).astype(np.int64)
    g = np.asarray(group, dtype=np.uint32)[rows].astype(np.int64)
    vals = np.ascontiguousarray(tab[s, zone])
    key = sort_key(vals, is_power)
    bkey = bound_keys(bounds, is_power)
    b1 = bkey.size + 1
    j = np.searchsorted(bkey, key, side="left")  # the bounds whose key is below the value's
    if is_power:
        nan = np.isnan(vals)
        add, dropped = fx(vals)
        unsummed = dropped & ~nan
    else:
        nan = np.zeros(vals.size, dtype=bool)
        add, unsummed = vals.astype(np.uint64), nan
    binned = ~nan
    out_bin = np.zeros((n_groups, b1), dtype=np.uint64)
    np.add.at(out_bin, (g[binned], j[binned]), np.uint64(1))
    out_sum = np.zeros(n_groups, dtype=np.uint64)
    with np.errstate(over="ignore"):
        np.add.at(out_sum, g[binned], add[binned])  # u64 adds wrap: the sum is mod 2^64
    out_nan = np.bincount(g[nan], minlength=n_groups).astype(np.uint64)
    out_uns = np.bincount(g[unsummed], minlength=n_groups).astype(np.uint64)
    return out_bin, np.cumsum(out_bin, axis=1, dtype=np.uint64), out_sum, out_nan, out_uns
