"""Plain reference of kacc_ticks_delta: the informer's arithmetic on Python integers, one row at a
time (populateProcessFields, informer.go:512-524; procWrapper.CPUTime, procfs_reader.go:75-82).

    prev = 0 for a NEW row, else map[slot]
    now  = (prev + inc) mod 2^64                      Go's uint sum
    Δ    = float(now) / 100.0 - float(prev) / 100.0   CPython's float(int) is correctly rounded,
                                                      `/` is one IEEE division
    map[slot] = now

A READ_ERROR node is skipped: its rows and its map slots are not touched.  The input is the wire
format of kepler_accel.h ("CPU-tick input format"), taken as it is: nothing here calls
accel.encode_ticks.  The documented errors are modelled too: a row whose slot is past the
capacity, and an escaped row that no valid escape of its node names, get Δ 0.0 and leave the map
alone; an escape is valid when it lies in its node's rows, names an escaped row and follows a
smaller row number; offsets past their arrays are cut to them.  Any of these sets the error bit.
"""

SLOT_NEW = 0x80000000
SLOT_MASK = 0x7FFFFFFF
ESCAPED = 0xFFFF
READ_ERROR = 0x1
M64 = (1 << 64) - 1
USER_HZ = 100.0


def cpu_time(ticks: int) -> float:
    """procWrapper.CPUTime: float64(STime + UTime) / userHZ."""
    return float(ticks) / USER_HZ


def cpu_delta(prev: int, now: int) -> float:
    return cpu_time(now) - cpu_time(prev)


class TicksRef:
    def __init__(self, slots: int):
        self.slots = slots
        self.map = [0] * slots

    def _row(self, word: int, inc: int):
        """(Δ, error) of one row with a valid increment; moves the map."""
        s = word & SLOT_MASK
        if s >= self.slots:
            return 0.0, True
        prev = 0 if word & SLOT_NEW else self.map[s]
        now = (prev + inc) & M64
        self.map[s] = now
        return cpu_delta(prev, now), False

    def delta(self, n_nodes, proc_off, proc_slot, dticks, esc_off=None, esc_row=(), esc_ticks=(), node_status=None):
        """One call.  Returns (delta, error): delta[r] is the float Δ of row r, or None for a row the
        call does not write (the rows of a skipped node); self.map is the map after the call."""
        P, E = len(proc_slot), len(esc_row)
        out = [None] * P
        err = False
        for n in range(n_nodes):
            if node_status is not None and int(node_status[n]) & READ_ERROR:
                continue
            p0, p1 = int(proc_off[n]), int(proc_off[n + 1])
            if p1 > P or p0 > p1:
                err = True
                p1 = min(p1, P)
                p0 = min(p0, p1)
            escaped = 0
            for r in range(p0, p1):
                if int(dticks[r]) == ESCAPED:
                    escaped += 1
                    out[r] = 0.0  # until its escape writes it
                    continue
                out[r], bad = self._row(int(proc_slot[r]), int(dticks[r]))
                err |= bad
            e0 = e1 = 0
            if E and esc_off is not None:
                e0, e1 = int(esc_off[n]), int(esc_off[n + 1])
                if e1 > E or e0 > e1:
                    err = True
                    e1 = min(e1, E)
                    e0 = min(e0, e1)
            if e1 - e0 != escaped:
                err = True
            for e in range(e0, e1):
                r = int(esc_row[e])
                if r < p0 or r >= p1 or int(dticks[r]) != ESCAPED or (e > e0 and int(esc_row[e - 1]) >= r):
                    err = True
                    continue
                out[r], bad = self._row(int(proc_slot[r]), int(esc_ticks[e]) & M64)
                err |= bad
        return out, err
