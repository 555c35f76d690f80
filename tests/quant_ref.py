"""The contract of kacc_group_quantiles (include/kepler_accel.h), restated in numpy.

Fed like tests/hist_ref.py: the table in the logical [slot * Z + zone] layout (the oracle's
``ora.state[...]`` or ``Accel.download``), the batch's offsets, slot words, node status, node mask
and group ids (None: every row in group 0) and phi as f64; returns the six outputs of one call.
numpy's f64 multiply and add are the IEEE operations of the header and ``astype(float64)`` of a u64
is correctly rounded, so a caller compares every output bit for bit.
"""

import numpy as np

from group_ref import contributing
from top_ref import KACC_SLOT_MASK, TOP, sort_key

KACC_QUANT_MAX_PHI = 8
KACC_QUANT_MAX_QUERIES = 65536
EMPTY_NAN = np.uint64(0x7FF8000000000001)  # out_value of a group without ranked rows


def phi_valid(phi):
    """The call's rule: 1 .. 8 values, each in [0, 1] (a NaN is not)."""
    f = np.ascontiguousarray(phi, dtype=np.float64)
    return bool(1 <= f.size <= KACC_QUANT_MAX_PHI and np.all((f >= 0.0) & (f <= 1.0)))


def key_bits(key, is_power):
    """The value bits a non-NaN key came from: key >= 1<<63 gives key & ~(1<<63) (either zero comes
    back as +0.0), otherwise ~key; an energy is its own key."""
    key = np.ascontiguousarray(key, dtype=np.uint64)
    if not is_power:
        return key.copy()
    return np.where(key >= TOP, key & ~TOP, ~key).astype(np.uint64)


def group_quantiles(table, is_power, zones, zone, row_off, slot_words, node_status, node_mask, group, n_groups, phi):
    """Expected outputs of one call.

    table is the state table [S * zones] (u64 energies or f64 powers).  A row whose slot is past the
    table is left out (the call also raises KACC_ERANGE for it, as for an id >= n_groups other than
    KACC_GROUP_NONE).  Returns (count u64 [G], nan u64 [G], lo u64 [G, P], hi u64 [G, P], weight f64
    [G, P], value f64 [G, P]) with P = len(phi)."""
    assert phi_valid(phi)
    phi = np.ascontiguousarray(phi, dtype=np.float64)
    assert n_groups * phi.size <= KACC_QUANT_MAX_QUERIES
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
    nan = np.isnan(vals) if is_power else np.zeros(vals.size, dtype=bool)
    out_nan = np.bincount(g[nan], minlength=n_groups).astype(np.uint64)
    g, key = g[~nan], key[~nan]
    order = np.lexsort((key, g))  # stable: by group, then ascending by key
    skey = key[order]
    count = np.bincount(g, minlength=n_groups).astype(np.int64)
    start = (np.cumsum(count) - count)[:, None]
    n = count[:, None]
    some = n > 0
    with np.errstate(invalid="ignore", over="ignore"):
        rank = phi[None, :] * (n - 1).astype(np.float64)  # one IEEE multiply
        floor = np.floor(rank)
        lower = np.where(some, floor, 0.0).astype(np.int64)
        upper = np.minimum(n - 1, lower + 1)
        weight = np.where(some, rank - floor, 0.0)
        padded = np.concatenate([skey, np.zeros(1, dtype=np.uint64)])  # an empty group reads the pad
        at = lambda pos: padded[np.where(some, start + pos, skey.size)]  # noqa: E731
        lo = np.where(some, key_bits(at(lower), is_power), np.uint64(0))
        hi = np.where(some, key_bits(at(upper), is_power), np.uint64(0))
        as_f64 = (lambda b: np.ascontiguousarray(b).view(np.float64)) if is_power else (lambda b: b.astype(np.float64))
        value = as_f64(lo) * (1.0 - weight) + as_f64(hi) * weight
    value = np.where(some, value.view(np.uint64), EMPTY_NAN).view(np.float64)
    return count.astype(np.uint64), out_nan, lo.astype(np.uint64), hi.astype(np.uint64), weight, value
