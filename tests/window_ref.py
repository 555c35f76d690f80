"""The contract of kacc_window_* (include/kepler_accel.h), restated in numpy.

A window over one workload kind: per slot the total at the window's start (``base``) and the group
of the slot's workload (``slot_group``), per group what the workloads that terminated inside the
window used in it (``retired``, ``retired_count``).  Fed like tests/group_ref.py: the kind's energy
table in the logical [slot * Z + zone] layout (the oracle's ``ora.state[...]`` or ``Accel.download``,
dense also for the pods) and the batch's offsets, slot words and node status.  Every sum is a u64
that wraps.  ``erange`` tells whether a call met an index the device reports as KACC_ERANGE.
"""

import numpy as np

KACC_SLOT_NEW = 0x80000000
KACC_SLOT_MASK = 0x7FFFFFFF
KACC_NODE_READ_ERROR = 0x1
KACC_GROUP_NONE = 0xFFFFFFFF
KACC_GROUP_MAX = 65536
KACC_WINDOW_ASSIGN_ALL = 0x1


class WindowRef:
    def __init__(self, slots, zones, n_groups):
        assert 1 <= n_groups <= KACC_GROUP_MAX
        self.S, self.Z, self.G = int(slots), int(zones), int(n_groups)
        self.base = np.zeros((self.S, self.Z), dtype=np.uint64)
        self.slot_group = np.full(self.S, KACC_GROUP_NONE, dtype=np.uint32)
        self.retired = np.zeros((self.G, self.Z), dtype=np.uint64)
        self.retired_count = np.zeros(self.G, dtype=np.uint32)
        self.erange = False
        self.reused = 0  # slots retired and adopted by one step, so far

    def _table(self, energy):
        return np.ascontiguousarray(np.asarray(energy, dtype=np.uint64).reshape(-1, self.Z))[:self.S]

    def _listed(self, row_off, n_rows, node_status, node_mask):
        """Bool [n_rows]: the rows of the nodes that list their rows - no read error, not masked out,
        a row range inside the batch (a range outside it is reported)."""
        row_off = np.asarray(row_off, dtype=np.int64)
        listed = np.zeros(n_rows, dtype=bool)
        for n in range(len(row_off) - 1):
            r0, r1 = int(row_off[n]), int(row_off[n + 1])
            if r0 > r1 or r1 > n_rows:
                self.erange = True
                continue
            if node_status is not None and int(node_status[n]) & KACC_NODE_READ_ERROR:
                continue
            if node_mask is not None and int(node_mask[n]) == 0:
                continue
            listed[r0:r1] = True
        return listed

    def step(self, energy, row_off, slot_words, node_status, group=None, flags=0, slot_off=None, term_slot=None,
             term_count=None):
        """One interval: (a) retire the join's terminated segments (term_count None: none), reading the
        tables as they stand before the interval; (b) adopt the listed NEW rows (every listed row
        under KACC_WINDOW_ASSIGN_ALL).  group None: every row in group 0 (n_groups 1)."""
        E = self._table(energy)
        retired_now = set()
        if term_count is not None:
            slot_off = np.asarray(slot_off, dtype=np.int64)
            for n in range(len(slot_off) - 1):
                c, b0 = int(term_count[n]), int(slot_off[n])
                if c > int(slot_off[n + 1]) - b0:  # the node's whole list is left out
                    self.erange = True
                    continue
                for s in np.asarray(term_slot[b0:b0 + c], dtype=np.int64).tolist():
                    if s >= self.S:
                        self.erange = True
                        continue
                    g = int(self.slot_group[s])
                    if g < self.G:
                        with np.errstate(over="ignore"):
                            self.retired[g] += E[s] - self.base[s]
                        self.retired_count[g] += 1
                        retired_now.add(s)
                    self.slot_group[s] = KACC_GROUP_NONE
        words = np.asarray(slot_words, dtype=np.uint32)
        n_rows = words.size
        if group is None:
            assert self.G == 1
            group = np.zeros(n_rows, dtype=np.uint32)
        group = np.asarray(group, dtype=np.uint32)
        listed = self._listed(row_off, n_rows, node_status, None)
        slots = (words & np.uint32(KACC_SLOT_MASK)).astype(np.int64)
        past = listed & (slots >= self.S)
        if past.any():
            self.erange = True
        fresh = listed & ~past & ((words & np.uint32(KACC_SLOT_NEW)) != 0)
        act = fresh | (listed & ~past) if flags & KACC_WINDOW_ASSIGN_ALL else fresh
        bad_id = act & (group >= np.uint32(min(self.G, 2**32 - 1))) & (group != np.uint32(KACC_GROUP_NONE))
        if bad_id.any():
            self.erange = True
        stored = np.where(group < np.uint32(min(self.G, 2**32 - 1)), group, np.uint32(KACC_GROUP_NONE))
        self.slot_group[slots[act]] = stored[act]
        self.base[slots[fresh]] = 0
        self.reused += len(retired_now & set(slots[fresh].tolist()))

    def mark(self, energy):
        """The window starts here: base = the totals, nothing retired; the groups stay."""
        self.base = self._table(energy).copy()
        self.retired[:] = 0
        self.retired_count[:] = 0

    def read(self, energy, row_off, slot_words, node_status, node_mask=None):
        """(count u32 [G], running u64 [G, Z], retired u64 [G, Z], retired_count u32 [G], total u64
        [G, Z], row u64 [n_rows, Z]) of one read after an interval."""
        E = self._table(energy)
        words = np.asarray(slot_words, dtype=np.uint32)
        listed = self._listed(row_off, words.size, node_status, node_mask)
        slots = (words & np.uint32(KACC_SLOT_MASK)).astype(np.int64)
        past = listed & (slots >= self.S)
        if past.any():
            self.erange = True
        ok = listed & ~past
        out_row = np.zeros((words.size, self.Z), dtype=np.uint64)
        s = slots[ok]
        with np.errstate(over="ignore"):
            out_row[ok] = E[s] - self.base[s]
        g = self.slot_group[s]
        grouped = g < np.uint32(min(self.G, 2**32 - 1))
        gi = g[grouped].astype(np.int64)
        count = np.bincount(gi, minlength=self.G).astype(np.uint32)
        running = np.zeros((self.G, self.Z), dtype=np.uint64)
        with np.errstate(over="ignore"):
            np.add.at(running, gi, out_row[ok][grouped])
            total = running + self.retired
        return count, running, self.retired.copy(), self.retired_count.copy(), total, out_row
