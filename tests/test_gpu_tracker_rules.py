"""kacc_tracker_add's retention and order rule under ties, sets past 512 and capacity overflow —
MI355X only.

The other tracker tests keep target-zone energies pairwise distinct.  Here they are tied, as a
tracker with min_energy 0 meets them (many short-lived processes end at 0 µJ), and the device is
compared with tests/tracker_ref.py — the documented rule: energy descending, tracked items before an
add's candidates, those in list order — after EVERY add, bit for bit: keys, nodes, every zone's
frozen energy, the frozen power's bits, and the order inside a node, through kacc_tracker_items and
through kacc_tracker_read.  tests/test_tracker_ref.py pins that model against the Go heap and checks
that these inputs reach the ties, the set sizes and the overflow they are meant to reach.

The tracker is driven through the C ABI as tests/test_gpu_tracker_export.py drives it: the kind's
tables uploaded, a SlotMap for slot_off, term_key / term_slot / term_count tensors, one launch per
add.  The expected power is the download of the kind's power table just before the add; between
adds the tables of the slots already listed are overwritten (tracker_cases.Scenario.tables).

Tried against one-token changes of node_add_wave_kernel: `>= se` -> `>` and `s_se[mid] > ei` -> `>=`
(rank searches) fail every tied test; the sort without its slot tie-break fails the tied tests of
more than a few candidates; `lds_set` forced true fails test_sets_past_512 and test_max_bounded.
The filter's `e <= min_full` -> `<` changes no output and cannot fail a test: a candidate at the
minimum of a full set ranks behind every tracked item and is cut, so `<=` only saves the work.
"""

import os
import re

import numpy as np
import pytest
import torch

import tracker_cases
from kepler_amd import accel
from kepler_amd.torch_batch import current_stream_handle
from oracle.oracle import OracleTracker
from tracker_ref import TrackerModel

pytestmark = pytest.mark.gpu

KIND_ID = {"proc": accel.KACC_KIND_PROC, "ctr": accel.KACC_KIND_CTR, "vm": accel.KACC_KIND_VM,
           "pod": accel.KACC_KIND_POD}
SENT64 = 0x5A5A5A5A5A5A5A5A  # output pre-fill: no key, energy or power bit pattern of these tests
SENT32 = 0x5A5A5A5A


@pytest.fixture(scope="module", autouse=True)
def gpu_ready():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    accel.load()
    torch.cuda.set_stream(torch.cuda.Stream())


class Device:
    """One context and one tracker; scenarios (one SlotMap each) run on it add by add."""

    def __init__(self, first, slots=None):
        s = first
        caps = {f"{k}_slots": 1 for k in KIND_ID}
        caps[f"{s.kind}_slots"] = slots or s.n_slots
        self.acc = accel.Accel(s.zones, nodes=s.n_nodes, **caps)
        self.tr = accel.Tracker(self.acc, KIND_ID[s.kind], s.max_size, zone=s.zone, min_energy=s.min_energy,
                                capacity=s.capacity)
        self.stream = current_stream_handle()

    def start(self, s):
        self.s = s
        self.sm = accel.SlotMap(self.acc, KIND_ID[s.kind], s.slot_off)
        self.model = TrackerModel(s.n_nodes, s.zones, s.zone, s.max_size, s.min_energy, s.capacity)

    def add(self, a):
        """Add a of the scenario on the device and in the model; returns the tables it read
        (energy [S, Z], power [S, Z] as downloaded)."""
        s = self.s
        t = s.tables(a)
        for name, v in t.items():
            self.acc.upload(name, v)
        e = t[f"{s.kind}_energy"].reshape(-1, s.zones)
        p = self.acc.download(f"{s.kind}_power", 0, s.n_slots * s.zones).reshape(-1, s.zones)
        np.testing.assert_array_equal(p.view(np.uint64), s.host_power(t).view(np.uint64))
        tk, ts, tc = s.term(a)
        self.model.add(s.slot_off, tk, ts, tc, e, p)
        self.term = [torch.from_numpy(x.view(d)).cuda() for x, d in ((tk, np.int64), (ts, np.int32), (tc, np.int32))]
        self.tr.add(self.sm, *[x.data_ptr() for x in self.term], self.stream)
        return e, p

    def items(self):
        k, nd, e, p = self.tr.items()
        return k.copy(), nd.copy(), e.copy(), p.view(np.uint64).copy()

    def read(self, total):
        """kacc_tracker_read into sentinel-filled outputs of total + 8 items: (node_off, key, node,
        energy, power bits), the 8 guard items checked here."""
        Z, N, cap = self.s.zones, self.s.n_nodes, total + 8
        d_off = torch.full((N + 1,), SENT32, dtype=torch.int32, device="cuda")
        d_key = torch.full((cap,), SENT64, dtype=torch.int64, device="cuda")
        d_node = torch.full((cap,), SENT32, dtype=torch.int32, device="cuda")
        d_e = torch.full((cap * Z,), SENT64, dtype=torch.int64, device="cuda")
        d_p = torch.full((cap * Z,), SENT64, dtype=torch.int64, device="cuda")
        self.tr.read(d_off.data_ptr(), cap, d_key.data_ptr(), d_node.data_ptr(), d_e.data_ptr(), d_p.data_ptr(),
                     stream=self.stream)
        self.acc.sync(self.stream)
        k, nd = d_key.cpu().numpy().view(np.uint64), d_node.cpu().numpy().view(np.uint32)
        e, p = (x.cpu().numpy().view(np.uint64).reshape(-1, Z) for x in (d_e, d_p))
        assert np.all(k[total:] == SENT64) and np.all(nd[total:] == SENT32)
        assert np.all(e[total:] == SENT64) and np.all(p[total:] == SENT64)
        return d_off.cpu().numpy().view(np.uint32), k[:total], nd[:total], e[:total], p[:total]

    def check(self, a, skip_nodes=()):
        """items() and read() against the model, bit for bit and in order (skip_nodes: compared by
        the caller)."""
        want = self.model.items()
        got = self.items()
        off, *dense = self.read(got[0].size)
        sizes = np.bincount(got[1], minlength=self.s.n_nodes)
        np.testing.assert_array_equal(off, np.r_[0, np.cumsum(sizes)].astype(np.uint32))
        for g, d in zip(got, dense):  # the two exports agree everywhere
            np.testing.assert_array_equal(g, d, err_msg=f"{self.s.name} add {a}: read != items")
        keep_g, keep_w = ~np.isin(got[1], skip_nodes), ~np.isin(want[1], skip_nodes)
        for what, g, w in zip(("key", "node", "energy", "power bits"), got, want):
            np.testing.assert_array_equal(g[keep_g], w[keep_w], err_msg=f"{self.s.name} add {a}: {what}")
        nd, ez = got[1].astype(np.int64), got[2][:, self.s.zone]
        assert np.all(np.diff(nd) >= 0)
        assert np.all(ez[1:][np.diff(nd) == 0] <= ez[:-1][np.diff(nd) == 0])  # descending, ties allowed
        return got

    def close(self):
        self.tr.close()
        self.acc.close()


def run(s, after_add=None):
    d = Device(s)
    d.start(s)
    for a in range(s.n_adds):
        d.add(a)
        got = d.check(a)
        if after_add:
            after_add(a, d, got)
    d.close()
    return d.model


@pytest.mark.parametrize("kind,zones,zone", tracker_cases.KINDS, ids=[k[0] for k in tracker_cases.KINDS])
def test_small_ties(kind, zones, zone):
    """max_size 5, energies from {1, 2, 3}, min_energy 0, 4 adds of 0 to 12 candidates, for every kind:
    proc (Z = 4) and ctr (Z = 1) run the <4> instance, vm Z = 3, pod (Z = 5) the 8-zone instance with
    table stride 2Z and a stored power; target zones 2, 0, 1, 3.  With them an all-zero node (keeps
    the first 5 by add order then list position, never evicts), the 101/102/103 pattern, and the
    order-independent already-tracked cases: the first copy and its frozen values stay."""
    s = tracker_cases.small_ties(kind, zones, zone)
    first = {}

    def relisted(a, d, got):
        k, nd, e, p = got
        if a == 0:  # the frozen values of the keys that are listed again later
            for n in (s.again_full, s.again_open):
                first.update({(n, int(kk)): (ee.copy(), pp.copy()) for kk, ee, pp in zip(k[nd == n], e[nd == n], p[nd == n])})
        for n, key in ((s.again_full, 303), (s.again_full, 304), (s.again_open, 401), (s.again_open, 402)):
            hit = (nd == n) & (k == key)
            assert hit.sum() == 1
            np.testing.assert_array_equal(e[hit][0], first[n, key][0])
            np.testing.assert_array_equal(p[hit][0], first[n, key][1])

    model = run(s, relisted)
    k, nd, _, _ = model.items()
    assert k[nd == s.pattern_node].tolist() == [201, 202, 203, 103, 101]  # 102, the newer tied minimum, went


def test_divergence_example():
    """max_size 2, adds of 101 (5 µJ), 102 (5 µJ), 103 (9 µJ): the device keeps {103, 101} (the Go
    heap {102, 103}, tests/test_tracker_ref.py)."""
    model = run(tracker_cases.divergence())
    assert model.items()[0].tolist() == [103, 101]


@pytest.mark.parametrize("kind,zones,zone", [("proc", 4, 2), ("pod", 5, 3)], ids=["proc", "pod"])
def test_ties_across_chunks_and_move_blocks(kind, zones, zone):
    """max_size 100, 4 distinct values, 3 adds of 200 per node: four 64-candidate chunks per add (the
    chunks must not show), a set of more than one 64-item move block."""
    run(tracker_cases.chunk_ties(kind, zones, zone))


@pytest.mark.parametrize("kind,zones,zone,tied", [("pod", 5, 3, True), ("proc", 4, 0, False), ("vm", 3, 1, True),
                                                  ("pod", 5, 0, False)],
                         ids=["tied-pod", "untied-proc", "tied-vm", "untied-pod"])
def test_sets_past_512(kind, zones, zone, tied):
    """max_size 1500, 6 adds of 300: the set passes 512 inside the second add — from there the rank
    searches and the moves read the tracked energies from global memory, not from the wave's LDS
    copy —, fills in the fifth and evicts in the sixth.  Tied: 8 distinct values.  Untied: also the
    Go heap's result exactly."""
    s = tracker_cases.big_sets(kind, zones, zone, tied)
    ora = OracleTracker(s.max_size, s.min_energy, s.zones, s.zone)
    d = Device(s)
    d.start(s)
    for a in range(s.n_adds):
        e, p = d.add(a)
        gk, gn, ge, gp = d.check(a)
        if not tied:
            tk, ts, tc = s.term(a)
            idx = np.concatenate([np.arange(s.slot_off[n], s.slot_off[n] + tc[n]) for n in range(s.n_nodes)]).astype(int)
            ora.add_batch(np.repeat(np.arange(s.n_nodes), tc), tk[idx], ts[idx], e, p)
            order = np.lexsort((gk, gn))
            ok, on, oe, op = ora.items()
            for g, o in ((gk, ok), (gn, on), (ge, oe), (gp, op.view(np.uint64))):
                np.testing.assert_array_equal(g[order], o, err_msg=f"{s.name} add {a}: Go heap")
    assert d.model.sizes().max() == 1500
    d.close()


def test_max_bounded():
    """One node at KACC_TRACKER_MAX_BOUNDED (max_size 8192, 3 adds of 4000, 50 distinct values);
    max_size 8193 is KACC_EINVAL."""
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "kepler_accel.h")).read()
    assert int(re.search(r"#define KACC_TRACKER_MAX_BOUNDED (\d+)u", header).group(1)) == 8192
    s = tracker_cases.max_bounded()
    model = run(s)
    assert model.sizes().tolist() == [8192]
    acc = accel.Accel(4, nodes=1, proc_slots=1, ctr_slots=1, vm_slots=1, pod_slots=1)
    with pytest.raises(accel.AccelError) as ei:
        accel.Tracker(acc, accel.KACC_KIND_PROC, 8193, zone=0, min_energy=0)
    assert ei.value.code == accel.KACC_EINVAL
    acc.close()


def test_threshold_edge():
    """min_energy m: a candidate at exactly m is kept, one at m - 1 is dropped; a max_size 0
    tracker's add returns OK and reads empty."""
    m = 1000
    s = tracker_cases.threshold(m)
    model = run(s)
    assert sorted(model.items()[2][:, s.zone].tolist()) == [m, m, m + 1, 2 * m]
    off = tracker_cases.threshold(m)
    off.max_size = 0
    d = Device(off)
    d.start(off)
    d.add(0)  # KACC_OK
    assert d.items()[0].size == 0
    node_off, k, _, _, _ = d.read(0)
    assert np.all(node_off == 0) and k.size == 0
    d.close()


def test_unlimited_overflow():
    """max_size -1, capacity 100: a node that receives 60 + 60 raises KACC_ERANGE at kacc_sync (bit
    1024, "tracker capacity") and holds exactly 100 of its candidates with their true frozen values,
    no duplicates, energies descending; every other node is the model's, exactly.  After a clear, the
    next add on the same tracker and context is exact again and raises nothing."""
    s, s2 = tracker_cases.overflow(), tracker_cases.after_overflow()
    assert (s.kind, s.zones, s.zone, s.n_nodes) == (s2.kind, s2.zones, s2.zone, s2.n_nodes)
    d = Device(s, slots=max(s.n_slots, s2.n_slots))
    d.start(s)
    d.add(0)
    d.check(0)  # 60 of 100: no error yet (check's read synchronizes)
    e, p = d.add(1)
    with pytest.raises(accel.AccelError, match="tracker capacity") as ei:
        d.acc.sync(d.stream)
    assert ei.value.code == accel.KACC_ERANGE and "bits 0x400:" in str(ei.value)  # that bit alone
    assert d.model.overflowed == {s.over_node}
    k, nd, ge, gp = d.check(1, skip_nodes=[s.over_node])
    n = s.over_node
    k, ge, gp = k[nd == n], ge[nd == n], gp[nd == n]
    assert k.size == 100 and np.unique(k).size == 100
    assert np.all(np.diff(ge[:, s.zone].astype(np.int64)) <= 0)
    # each item is one of the node's candidates, with the values its add read
    e0 = s.tables(0)[f"{s.kind}_energy"].reshape(-1, s.zones)
    p0 = s.host_power(s.tables(0))
    lo, mid, hi = int(s.start[0, n]), int(s.start[1, n]), int(s.start[1, n] + s.count[1, n])
    truth = {int(s.key[i]): (e0[i], p0[i].view(np.uint64)) for i in range(lo, mid)}
    truth.update({int(s.key[i]): (e[i], p[i].view(np.uint64)) for i in range(mid, hi)})
    for kk, ee, pp in zip(k, ge, gp):
        np.testing.assert_array_equal(ee, truth[int(kk)][0])
        np.testing.assert_array_equal(pp, truth[int(kk)][1])
    # the same tracker and context afterwards
    d.tr.clear(d.stream)
    d.start(s2)
    d.add(0)
    d.check(0)
    d.acc.sync(d.stream)
    assert not d.model.overflowed and d.model.sizes().tolist() == [0, 70, 100, 1, 30]
    d.close()
