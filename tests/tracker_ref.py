"""The retention and order rule of kacc_tracker_add (include/kepler_accel.h), restated in plain Python.

A node's set is a list ordered by (target-zone energy descending, then insertion order).  One add,
per node: candidates whose key is in the set when the add starts are dropped (:90), then those
below min_energy (:102); the rest are stable-sorted by (energy descending, position in the node's
terminated list), placed behind the tracked items of equal energy, and the list is cut to max_size
(an unlimited tracker: to its per-node capacity, which flags the overflow).  Every item is a frozen
copy, taken at add time, of its slot's per-zone energy and power.

Fed from the kind's tables in the logical [slot, zone] layout (``Accel.download`` reshaped, or the
arrays a test uploads) and the add's term_key / term_slot / term_count arrays.  No heap and no
chunks: the result is a function of the set and the list alone.
"""

import numpy as np


class TrackerModel:
    def __init__(self, n_nodes, zones, zone, max_size, min_energy=0, capacity=0):
        self.n_nodes, self.zones, self.zone = n_nodes, zones, zone
        self.max_size, self.min_energy, self.capacity = max_size, min_energy, capacity
        # per node: [target-zone energy (int), key (int), energy u64 [Z], power f64 [Z]], in set order
        self.sets = [[] for _ in range(n_nodes)]
        self.overflowed = set()     # nodes of an unlimited tracker that were cut to the capacity
        self.boundary_tied = set()  # nodes where an item was dropped at the energy of the last one kept

    def clear(self, nodes=None):
        for n in range(self.n_nodes) if nodes is None else nodes:
            self.sets[n] = []

    def add(self, slot_off, term_key, term_slot, term_count, tab_e, tab_p):
        """slot_off [N + 1]; term_key / term_slot [slot_off[N]] and term_count [N]: node n's list at
        [slot_off[n], slot_off[n] + term_count[n]); tab_e u64 / tab_p f64: [S, Z], read now."""
        if self.max_size == 0:
            return
        tab_e = np.asarray(tab_e, dtype=np.uint64).reshape(-1, self.zones)
        tab_p = np.asarray(tab_p, dtype=np.float64).reshape(-1, self.zones)
        keep = self.max_size if self.max_size > 0 else self.capacity
        for n in range(self.n_nodes):
            b0, items = int(slot_off[n]), self.sets[n]
            tracked = {it[1] for it in items}
            cand = []
            for i in range(b0, b0 + int(term_count[n])):
                key, slot = int(term_key[i]), int(term_slot[i])
                e = int(tab_e[slot, self.zone])
                if key in tracked or e < self.min_energy:
                    continue
                cand.append([e, key, tab_e[slot].copy(), tab_p[slot].copy()])
            cand.sort(key=lambda it: -it[0])  # stable: list position breaks ties
            merged = sorted(items + cand, key=lambda it: -it[0])  # stable: tracked before the batch
            if len(merged) > keep:
                if self.max_size < 0:
                    self.overflowed.add(n)
                if keep and merged[keep][0] == merged[keep - 1][0]:
                    self.boundary_tied.add(n)
            self.sets[n] = merged[:keep]

    def items(self):
        """(key u64 [n], node u32 [n], energy u64 [n, Z], power BITS u64 [n, Z]): node by node, each
        node's items in set order — what kacc_tracker_items and kacc_tracker_read return."""
        rows = [(n, it) for n in range(self.n_nodes) for it in self.sets[n]]
        key = np.array([it[1] for _, it in rows], dtype=np.uint64)
        node = np.array([n for n, _ in rows], dtype=np.uint32)
        e = np.array([it[2] for _, it in rows], dtype=np.uint64).reshape(-1, self.zones)
        p = np.array([it[3] for _, it in rows], dtype=np.float64).reshape(-1, self.zones)
        return key, node, e, p.view(np.uint64)

    def sizes(self):
        return np.array([len(s) for s in self.sets], dtype=np.int64)
