"""Directed edge cases of kacc_ticks_delta against tests/ticks_ref.py — MI355X only.

Δ and the tick map are compared as u64 bits, every Δ finite: float64(uint64) at its rounding ties
(2^53.., 2^63.., 2^64-1), the IEEE division by 100 at every tick count 1..4096, prev = 0 for a NEW
row in the regular and the escape path; node row counts on the kernel's tiling (256 threads x 4
rows = 1024 rows per pass); READ_ERROR nodes left untouched (rows and map slots); and every
documented error, one defect per run on a small healthy batch.
"""

import copy

import numpy as np
import pytest
import torch

from kepler_amd import accel
from kepler_amd.torch_batch import current_stream_handle
from ticks_ref import ESCAPED, READ_ERROR, SLOT_NEW, TicksRef

pytestmark = pytest.mark.gpu

SENTINEL = 0xC0DEC0DEC0DEC0DE  # a finite double no Δ here equals: a row the call did not write
M64 = (1 << 64) - 1
_VIEW = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}


@pytest.fixture(scope="module", autouse=True)
def gpu_ready():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    accel.load()
    torch.cuda.set_stream(torch.cuda.Stream())


def _dev(a, dt):
    a = np.ascontiguousarray(a, dtype=dt)
    return torch.from_numpy(a.view(_VIEW.get(a.dtype, a.dtype))).cuda()


def _i64(v):
    """An increment as the int64 of esc_ticks (values >= 2^63 sent as negative)."""
    v &= M64
    return v - (1 << 64) if v >= 1 << 63 else v


class Batch:
    """One call's input in the wire format, built from per-row increments (Python ints)."""

    def __init__(self, counts, slots, new, incs, escaped=None, node_status=None, with_esc_off=True):
        self.n_nodes = len(counts)
        self.proc_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
        P = int(self.proc_off[-1])
        assert len(slots) == P and len(incs) == P
        new = np.broadcast_to(np.asarray(new, dtype=bool), (P,))
        self.proc_slot = (np.asarray(slots, dtype=np.uint32) | np.where(new, np.uint32(SLOT_NEW), np.uint32(0)))
        esc = np.array([not 0 <= i < ESCAPED for i in incs], dtype=bool)
        if escaped is not None:  # rows sent as escapes although their increment would fit
            esc |= np.asarray(escaped, dtype=bool)
        self.dticks = np.array([ESCAPED if e else i for i, e in zip(incs, esc)], dtype=np.uint16)
        self.esc_row = np.flatnonzero(esc).astype(np.uint32)
        self.esc_ticks = np.array([_i64(incs[r]) for r in self.esc_row], dtype=np.int64)
        self.esc_off = np.searchsorted(self.esc_row, self.proc_off).astype(np.uint32) if with_esc_off else None
        self.node_status = None if node_status is None else np.asarray(node_status, dtype=np.uint32)


class Device:
    def __init__(self, node_cap, slots):
        self.acc = accel.Accel(1, nodes=node_cap, proc_slots=slots, ctr_slots=1, vm_slots=1, pod_slots=1)
        self.tm = accel.TickMap(self.acc)
        self.ref = TicksRef(slots)

    def run(self, b, label):
        """The call on the device and in the reference: the error code, every Δ (an unwritten row
        keeps the sentinel) and the whole map must agree.  Returns (Δ bits, error code)."""
        s = current_stream_handle()
        P, E = b.proc_slot.size, b.esc_row.size
        t = {"off": _dev(b.proc_off, np.uint32), "slot": _dev(b.proc_slot, np.uint32), "dt": _dev(b.dticks, np.uint16)}
        if b.esc_off is not None:
            t["eo"] = _dev(b.esc_off, np.uint32)
        if E:
            t["er"], t["ev"] = _dev(b.esc_row, np.uint32), _dev(b.esc_ticks, np.int64)
        if b.node_status is not None:
            t["st"] = _dev(b.node_status, np.uint32)
        out = torch.from_numpy(np.full(P, SENTINEL, dtype=np.uint64).view(np.int64)).cuda()
        ptr = lambda k: t[k].data_ptr() if k in t else None  # noqa: E731
        tk = accel.KaccTicks(b.n_nodes, P, E, 0, ptr("off"), ptr("st"), ptr("slot"), ptr("dt"), ptr("eo"), ptr("er"),
                             ptr("ev"), out.data_ptr())
        self.tm.delta(tk, s)
        code = accel.KACC_OK
        try:
            self.acc.sync(s)
        except accel.AccelError as e:
            code = e.code
        got = out.cpu().numpy().view(np.uint64)
        want, err = self.ref.delta(b.n_nodes, b.proc_off, b.proc_slot, b.dticks, b.esc_off, b.esc_row, b.esc_ticks,
                                   b.node_status)
        bits = np.array([0.0 if w is None else w for w in want], dtype=np.float64).view(np.uint64).copy()
        bits[[w is None for w in want]] = SENTINEL
        assert np.isfinite(bits.view(np.float64)).all()
        assert code == (accel.KACC_ERANGE if err else accel.KACC_OK), label
        np.testing.assert_array_equal(got, bits, err_msg=f"{label}: delta")
        np.testing.assert_array_equal(self.tm.download(), np.array(self.ref.map, dtype=np.uint64),
                                      err_msg=f"{label}: tick map")
        return got, code

    def close(self):
        self.tm.close()
        self.acc.close()


ROUNDING = [2**53 - 1, 2**53, 2**53 + 1, 2**53 + 3, 2**54 + 2, 2**54 + 6,
            2**63 + 2**10, 2**63 + 2**10 + 1, 2**63 + 3 * 2**10,
            2**64 - 1025, 2**64 - 1024, 2**64 - 1,
            (0x200001 << 32) | 0x80000000, (0x200000 << 32) | 0x80000000, (0x3FFFFF << 32) | 0xFFFFFFFF]


def test_rounding_of_ticks_and_division_by_100():
    """One node.  Interval 1: NEW rows whose increment is each rounding value (four rows each) and
    every tick count 1..4096, once through an escape and once as a regular u16 increment.
    Interval 2: the same slots, not NEW, increments 0, 1, 2, 0xfffe (every other group of four as
    escapes): prev and now both round, 2^64-1 plus 1 wraps to 0.  Interval 3: interval 1 again,
    NEW on slots whose entry is not 0: prev must be 0 in both paths."""
    rng = np.random.default_rng(53)
    now = [v for v in ROUNDING for _ in range(4)] + list(range(1, 4097)) * 2
    as_escape = np.array([True] * (len(ROUNDING) * 4 + 4096) + [False] * 4096)
    step = [(0, 1, 2, 0xFFFE)[i % 4] for i in range(len(now))]
    P = len(now)
    order = rng.permutation(P)  # escapes and regular rows mixed over the node's tiles
    now, step, as_escape = [now[i] for i in order], [step[i] for i in order], as_escape[order]
    slots = rng.permutation(P + 5)[:P]
    d = Device(1, P + 5)
    first, _ = d.run(Batch([P], slots, True, now, as_escape), "interval 1")
    want1 = np.array([float(v) / 100.0 for v in now]).view(np.uint64)  # NEW: Δ = float64(now)/100 - 0
    np.testing.assert_array_equal(first, want1)
    d.run(Batch([P], slots, False, step, [(i // 4) % 2 == 1 for i in range(P)]), "interval 2")
    wrapped = [int(slots[i]) for i in range(P) if now[i] == 2**64 - 1 and step[i] == 1]
    assert len(wrapped) == 1 and d.tm.download()[wrapped[0]] == 0
    assert np.count_nonzero(d.tm.download()[slots]) == P - 1
    third, _ = d.run(Batch([P], slots, True, now, as_escape), "interval 3")
    np.testing.assert_array_equal(third, first)
    d.close()


TILE_COUNTS = [0, 0, 1, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 257, 0]
ALL_ESCAPED_NODE = 12


def _tiling_escapes(counts):
    esc = []
    for n, c in enumerate(counts):
        e = np.zeros(c, dtype=bool)
        e[[r for r in (0, c - 1, 255, 256, 1023, 1024) if 0 <= r < c]] = True
        if n == ALL_ESCAPED_NODE:
            e[:] = True
        esc.append(e)
    return np.concatenate(esc)


def test_node_sizes_on_the_kernel_tiling():
    rng = np.random.default_rng(1024)
    counts = TILE_COUNTS
    P = sum(counts)
    off = np.concatenate([[0], np.cumsum(counts)])
    slots = np.concatenate([3 + off[n] + rng.permutation(c) for n, c in enumerate(counts)])  # shuffled inside each node
    esc = _tiling_escapes(counts)
    d = Device(len(counts) + 2, P + 8)  # n_nodes below the context's capacity
    # A: NEW rows; the marked rows carry big first readings
    inc = [int(rng.integers(0xFFFF, 1 << 62)) if e else int(rng.integers(0, 0xFFFF)) for e in esc]
    d.run(Batch(counts, slots, True, inc, esc, node_status=np.zeros(len(counts))), "A")
    # B: the same slots again, node_status NULL; the marked rows go back or jump
    inc = [(-int(rng.integers(1, 1 << 40)) if rng.random() < 0.5 else int(rng.integers(0xFFFF, 1 << 63))) if e
           else int(rng.integers(0, 0xFFFF)) for e in esc]
    b = Batch(counts, slots, False, inc, esc)
    assert b.esc_row.size == esc.sum() and np.diff(b.esc_off)[ALL_ESCAPED_NODE] == counts[ALL_ESCAPED_NODE]
    d.run(b, "B")
    # C: no escapes at all, esc_off NULL
    inc = [int(rng.integers(0, 0xFFFF)) for _ in range(P)]
    inc[:: 97] = [0xFFFE] * len(inc[:: 97])
    c = Batch(counts, slots, False, inc, with_esc_off=False)
    assert c.esc_row.size == 0 and c.esc_off is None
    d.run(c, "C")
    d.close()


def test_read_error_nodes_are_left_untouched():
    rng = np.random.default_rng(399)
    counts = [300, 5, 1025, 64, 0, 700]
    P = sum(counts)
    off = np.concatenate([[0], np.cumsum(counts)])
    slots = rng.permutation(P + 3)[:P]
    d = Device(len(counts), P + 3)
    inc = [int(rng.integers(1, 1 << 50)) if rng.random() < 0.1 else int(rng.integers(1, 3000)) for _ in range(P)]
    d.run(Batch(counts, slots, True, inc), "first readings")
    before = d.tm.download()
    status = np.zeros(len(counts), dtype=np.uint32)
    status[[1, 2]] = READ_ERROR
    inc = [int(rng.integers(1, 3000)) for _ in range(P)]
    for r in (off[2], off[2] + 511, off[3] - 1, off[0] + 7, off[5] + 699):  # node 2 has escapes of its own
        inc[r] = -5
    b = Batch(counts, slots, False, inc, node_status=status)
    assert np.diff(b.esc_off).tolist() == [1, 0, 3, 0, 0, 1]
    got, _ = d.run(b, "two nodes skipped")
    skipped = np.zeros(P, dtype=bool)
    skipped[off[1]:off[3]] = True
    assert (got[skipped] == SENTINEL).all() and (got[~skipped] != SENTINEL).all()
    after = d.tm.download()
    np.testing.assert_array_equal(after[slots[skipped]], before[slots[skipped]])
    assert (after[slots[~skipped]] != before[slots[~skipped]]).all()  # every increment here is not 0
    d.run(Batch(counts, slots, False, [int(rng.integers(0, 3000)) for _ in range(P)]), "all nodes again")
    d.close()


# ---- errors: a small healthy batch with one defect ------------------------------------------
ERR_COUNTS = [40, 30, 20]
ERR_SLOTS = 100
ERR_ESCAPED = [3, 17, 45, 80, 85]  # rows sent as escapes (nodes 0, 0, 1, 2, 2)


def _slot_regular(b):
    b.proc_slot[10] = ERR_SLOTS
    return [10]


def _slot_escaped(b):
    b.proc_slot[17] = ERR_SLOTS + 5
    return [17]


def _proc_off_past_n_procs(b):
    b.proc_off[3] = 97
    return []


def _proc_off_decreasing(b):
    b.proc_off[3] = 60  # node 2: [70, 60) — no rows; its escapes have no node
    return []


def _esc_off_past_n_escapes(b):
    b.esc_off[3] = 8
    return []


def _escape_in_another_node(b):
    b.esc_row[2] = 75  # node 1's only escape names a row of node 2
    return [45]


def _escape_names_a_regular_row(b):
    b.esc_row[0] = 2
    return [3]


def _same_row_twice(b):
    b.esc_row[1] = 3
    return [17]


def _one_escape_too_many(b):
    b.esc_row = np.array([3, 17, 45, 50, 80, 85], dtype=np.uint32)  # row 50 is a regular row
    b.esc_ticks = np.insert(b.esc_ticks, 3, 70000)
    b.esc_off = np.array([0, 2, 4, 6], dtype=np.uint32)
    return []


def _one_escape_too_few(b):
    b.esc_row, b.esc_ticks = b.esc_row[:4].copy(), b.esc_ticks[:4].copy()
    b.esc_off = np.array([0, 2, 3, 4], dtype=np.uint32)
    return [85]


DEFECTS = [_slot_regular, _slot_escaped, _proc_off_past_n_procs, _proc_off_decreasing, _esc_off_past_n_escapes,
           _escape_in_another_node, _escape_names_a_regular_row, _same_row_twice, _one_escape_too_many,
           _one_escape_too_few]


@pytest.mark.parametrize("defect", DEFECTS, ids=lambda f: f.__name__.strip("_"))
def test_one_defect_raises_erange_and_spares_the_rest(defect):
    """Every load and store of ticks_kernel is bounded for these inputs (offsets cut to n_procs /
    n_escapes, map[0] read for a bad slot, an escape's row checked against its node before
    dticks[row]); the arrays keep their declared lengths, only values are wrong."""
    rng = np.random.default_rng(7)
    P = sum(ERR_COUNTS)
    slots = rng.permutation(ERR_SLOTS)[:P]
    d = Device(len(ERR_COUNTS), ERR_SLOTS)
    esc = np.zeros(P, dtype=bool)
    esc[ERR_ESCAPED] = True

    def healthy(new):
        inc = [int(rng.integers(1, 3000)) for _ in range(P)]
        for r in ERR_ESCAPED:
            inc[r] = int(rng.integers(0x10000, 1 << 40))
        return Batch(ERR_COUNTS, slots, new, inc, esc)

    _, code = d.run(healthy(True), "first readings")
    assert code == accel.KACC_OK
    b = copy.deepcopy(healthy(False))
    zero_rows = defect(b)
    got, code = d.run(b, defect.__name__)  # compares every row and the whole map with the reference
    assert code == accel.KACC_ERANGE
    assert (got[zero_rows] == 0).all()  # Δ = +0.0 for the rows the header names
    _, code = d.run(healthy(False), "clean call after the error")
    assert code == accel.KACC_OK
    d.close()
