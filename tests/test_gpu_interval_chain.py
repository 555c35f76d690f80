"""The node workgroup's chain of dependent loads (interval_node) — MI355X only.

interval_kernel / interval_sums_kernel order a node's loads so that no wait drains the loads
in flight: the aggregate capacities and table pointers stay scalar, Δ and the slot words go
to LDS as they land.  None of it may change a bit: every state table is compared with the
oracle after every interval, at the node sizes at the edges of the row paths (1, 63, 64, 65,
512, 2047, 2048 rows), at the aggregate counts at which a 10-KiB LDS area for the aggregates'
previous totals fills and overflows (DESIGN §10 lists that piece, the per-node slot
prediction and the one-division-per-row piece as rejected; their cases stay), and through
the ways a node's slots move between intervals: shifted slots, one row moved away, a skipped
node, NEW rows inside a group, kacc_reset, a table upload, another node's slot range, the
end of a proc_slots capacity that is no multiple of 64, a node that grew.
"""

import numpy as np
import pytest
import torch

from kepler_amd import accel, fleet
from kepler_amd.torch_batch import current_stream_handle, interval_from_tensors, to_device
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu

ARENA_WORDS = 2 * 512 + 256  # 8-byte words of a 10-KiB LDS area for the aggregates' previous totals
PAD = 200                    # free slots after each node's range (room for the shifts)
NEW = np.uint32(accel.KACC_SLOT_NEW)


@pytest.fixture(scope="module", autouse=True)
def gpu_ready():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    accel.load()
    torch.cuda.set_stream(torch.cuda.Stream())


def fit(zones):
    """The most aggregates per node whose previous totals (8Z bytes each) fit that area."""
    return min(512, ARENA_WORDS // zones)


def node_spec(rows, aggs):
    """A node of `rows` processes and `aggs` aggregates: containers (some empty when there are
    more of them than rows), one VM from four aggregates on, pods over a third."""
    nvm = 1 if aggs >= 4 else 0
    npod = aggs // 3
    nctr = aggs - nvm - npod
    in_ctr = rows * 3 // 4 if nctr else 0
    ctr = [in_ctr // nctr + (1 if c < in_ctr % nctr else 0) for c in range(nctr)]
    podded = nctr - 1 if nctr > 1 else nctr  # the last container stays pod-less
    pod = [podded // npod + (1 if q < podded % npod else 0) for q in range(npod)]
    return dict(rows=rows, ctr=ctr, vm=[min(rows - in_ctr, 3)] * nvm, pod=pod)


def fleets(zones):
    """Two six-node fleets: every row count and every aggregate count of the edges."""
    f, g = fit(zones), min(fit(zones) + 1, 512)
    return [
        [(2048, f), (63, 0), (64, 1), (512, g), (1, 1), (2047, 512)],
        [(65, g), (2048, 512), (2047, 0), (64, f), (512, 1), (63, 0)],
    ]


class Plans:
    """Row -> slot maps of one layout: each node's rows at consecutive slots from its base."""

    def __init__(self, layout, cap=None):
        self.off = layout.proc_off.astype(np.int64)
        self.rows = np.diff(self.off)
        n = len(self.rows)
        self.base = 70 + np.concatenate([[0], np.cumsum(self.rows + PAD)[:-1]])
        self.far = int(self.base[-1] + self.rows[-1] + PAD)  # distant slots, one per node
        end = self.far + n + 64
        self.cap = cap if cap is not None else end + 33 + (1 if (end + 33) % 64 == 0 else 0)
        assert self.cap % 64 != 0 and self.cap >= end + 33

    def _from(self, base):
        return np.concatenate([b + np.arange(r) for b, r in zip(base, self.rows)]).astype(np.uint32)

    def at(self, shift=0):
        return self._from(self.base + shift)

    def one_row_away(self, shift=0):
        """(b) row 10 of every node with a full group moves to a distant slot."""
        s = self.at(shift)
        for n in np.flatnonzero(self.rows >= 64):
            s[self.off[n] + 10] = self.far + n
        return s

    def reversed_ranges(self):
        """(f) the nodes' ranges in reverse node order: a node's old slots are another node's rows."""
        order = np.arange(len(self.rows))[::-1]
        base = np.zeros(len(self.rows), dtype=np.int64)
        base[order] = 70 + np.concatenate([[0], np.cumsum(self.rows[order] + PAD)[:-1]])
        assert np.any(base != self.base)
        return self._from(base)

    def node_at_end(self, n):
        """(g) node n's rows end at the last slot of the table."""
        base = self.base.copy()
        base[n] = self.cap - self.rows[n]
        return self._from(base)


class Live:
    """Slots whose derived process power is the reference's: attributed by their node at that
    node's last processed interval (tests/table_check.py)."""

    def __init__(self, cap):
        self.owner = np.full(cap, -1, dtype=np.int64)
        self.valid = np.zeros(cap, dtype=bool)

    def update(self, proc_off, slots, status):
        ok = (np.asarray(status) & accel.KACC_NODE_READ_ERROR) == 0
        self.valid[np.isin(self.owner, np.flatnonzero(ok))] = False
        node = np.repeat(np.arange(len(ok)), np.diff(proc_off.astype(np.int64)))
        keep = ok[node]
        s = (slots[keep] & np.uint32(accel.KACC_SLOT_MASK)).astype(np.int64)
        self.owner[s] = node[keep]
        self.valid[s] = True


def check_tables(acc, ora, live, zones, msg):
    for name, _ in accel.TABLES:
        got, want = acc.download(name), ora.state[name]
        if name == "proc_power":
            m = np.repeat(live.valid, zones)
            got, want = got[m], want[m]
        if want.dtype == np.float64:  # any NaN equals any NaN (test_gpu_parity.assert_table_equal)
            bad = (got.view(np.uint64) != want.view(np.uint64)) & ~(np.isnan(got) & np.isnan(want))
            assert not bad.any(), f"{msg} {name}: {int(bad.sum())} differ, first at {int(np.flatnonzero(bad)[0])}"
        else:
            np.testing.assert_array_equal(got, want, err_msg=f"{msg} {name}")


class Pair:
    """The engine and the oracle fed the same intervals."""

    def __init__(self, zones, caps):
        self.zones, self.caps = zones, caps
        self.acc = accel.Accel(zones, **caps)
        self.ora = Oracle(zones, **caps)
        self.live = Live(caps["proc_slots"])
        self.k = 0

    def step(self, layout, a, slots, what, new_rows=None, skip=None):
        a = dict(a)
        words = slots | (a["proc_slot"] & NEW)
        if new_rows is not None:
            words[new_rows] |= NEW
        a["proc_slot"] = words
        if skip is not None:
            a["node_status"] = a["node_status"].copy()
            a["node_status"][skip] |= np.uint32(accel.KACC_NODE_READ_ERROR)
        s = current_stream_handle()
        t = to_device(a)
        self.acc.run_interval(interval_from_tensors(t, layout.sizes(), layout.fast_flag()), s)
        self.acc.sync(s)
        self.ora.interval(a, layout.sizes())
        self.live.update(layout.proc_off, words, a["node_status"])
        check_tables(self.acc, self.ora, self.live, self.zones, f"interval {self.k} ({what})")
        self.k += 1

    def reset(self):
        self.acc.reset()
        self.ora = Oracle(self.zones, **self.caps)
        self.live = Live(self.caps["proc_slots"])

    def upload_proc_energy(self, rng):
        v = rng.integers(0, 1 << 40, size=self.ora.state["proc_energy"].size).astype(np.uint64)
        self.acc.upload("proc_energy", v, 0)
        self.ora.state["proc_energy"][:] = v


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("zones", [1, 2, 3, 4, 5, 8])
def test_interval_chain_bit_exact(zones, which):
    spec = fleets(zones)[which]
    L1 = fleet.layout_from_sizes(zones, [node_spec(r, g) for r, g in spec], seed=41)
    L2 = fleet.layout_from_sizes(zones, [node_spec(r, g) for r, g in spec[::-1]], seed=42)  # nodes grow / shrink
    assert L1.fast_flag() & accel.KACC_F_FAST_NODES and not L1.fast_flag() & accel.KACC_F_SMALL_NODES
    p1 = Plans(L1)
    p2 = Plans(L2, cap=p1.cap)
    caps = L1.capacities()
    assert caps == L2.capacities()
    caps["proc_slots"] = p1.cap
    pair = Pair(zones, caps)
    sim = fleet.FleetSim(L1, seed=41, churn=0.03, zero_ratio_frac=0.0)
    rows = p1.rows
    mid = np.concatenate([p1.off[n] + np.array([20, 21, 40]) for n in np.flatnonzero(rows >= 64)])  # (d)
    skipped = int(np.flatnonzero(rows == 2048)[0])
    last64 = int(np.flatnonzero(rows == 64)[0])
    assert np.diff(L2.proc_off.astype(np.int64))[last64] >= 128  # the node at the table's end grows

    pair.step(L1, sim.next_interval(), p1.at(), "first read")
    pair.step(L1, sim.next_interval(), p1.at(), "the same slots")
    pair.step(L1, sim.next_interval(), p1.at(37), "a: every slot shifted")
    pair.step(L1, sim.next_interval(), p1.at(37), "c: a node skipped", skip=skipped)
    pair.step(L1, sim.next_interval(), p1.at(37), "c: the skipped node is back")
    pair.step(L1, sim.next_interval(), p1.one_row_away(37), "b + d: one row away, NEW rows in a group", new_rows=mid)
    pair.step(L1, sim.next_interval(), p1.at(), "back at the first slots")
    pair.step(L1, sim.next_interval(), p1.at(), "the same slots again")
    pair.step(L1, sim.next_interval(), p1.reversed_ranges(), "f: every node in another node's slot range")
    pair.reset()
    pair.step(L1, sim.next_interval(), p1.at(), "e: after kacc_reset")
    pair.upload_proc_energy(np.random.default_rng(zones))
    pair.step(L1, sim.next_interval(), p1.at(), "e: after a proc_energy upload")
    pair.step(L1, sim.next_interval(), p1.node_at_end(last64), "g: a node at the table's end")
    assert int(p1.node_at_end(last64)[p1.off[last64]]) + 64 == p1.cap
    sim2 = fleet.FleetSim(L2, seed=42, churn=0.03, zero_ratio_frac=0.0)
    pair.step(L2, sim2.next_interval(), p2.at(), "g: that node grew and moved")
    pair.step(L2, sim2.next_interval(), p2.at(), "the grown layout again")
    pair.acc.close()


def test_interval_chain_through_interval_sums():
    """interval_sums_kernel shares interval_node: pod and node exports of every interval, the
    namespace totals of the last one against kor_namespace_totals."""
    zones = 4
    L = fleet.layout_from_sizes(zones, [node_spec(r, g) for r, g in fleets(zones)[0]], seed=43)
    p = Plans(L)
    caps = L.capacities()
    caps["proc_slots"] = p.cap
    acc = accel.Accel(zones, **caps)
    ora = Oracle(zones, **caps)
    live = Live(p.cap)
    sim = fleet.FleetSim(L, seed=43, churn=0.03, zero_ratio_frac=0.0)
    s = current_stream_handle()
    n_ns = L.n_namespaces
    off, slots_ns = L.namespace_csr()
    _, rows_ns = L.namespace_csr_rows()
    d = to_device({"o": off, "r": rows_ns})
    pex = [torch.zeros(max(L.n_pods, 1) * 2 * zones, dtype=torch.int64, device="cuda") for _ in range(2)]
    nex = [torch.zeros(L.n_nodes * 5 * zones, dtype=torch.int64, device="cuda") for _ in range(2)]
    out_e = torch.zeros(n_ns * zones, dtype=torch.int64, device="cuda")
    out_p = torch.zeros(n_ns * zones, dtype=torch.float64, device="cuda")
    out_ne = torch.zeros(2 * zones, dtype=torch.int64, device="cuda")
    out_np = torch.zeros(3 * zones, dtype=torch.float64, device="cuda")

    def sums_of(k):
        x = accel.KaccExportSums()
        x.n_ns, x.n_pods, x.n_nodes, x.ns_ordered = n_ns, L.n_pods, L.n_nodes, 0
        x.ns_pod_off, x.ns_pod_row = d["o"].data_ptr(), d["r"].data_ptr()
        x.pod_export, x.node_export = pex[k % 2].data_ptr(), nex[k % 2].data_ptr()
        x.out_energy, x.out_power = out_e.data_ptr(), out_p.data_ptr()
        x.out_node_energy, x.out_node_power = out_ne.data_ptr(), out_np.data_ptr()
        return x

    plans = [p.at(), p.at(), p.at(37), p.one_row_away(37), p.at(37)]
    keep = []
    for k, slots in enumerate(plans):
        a = sim.next_interval()
        a["proc_slot"] = slots | (a["proc_slot"] & NEW)
        t = to_device(a)
        t["pod_export"], t["node_export"] = pex[k % 2], nex[k % 2]
        keep.append(t)
        acc.run_interval_sums(interval_from_tensors(t, L.sizes(), L.fast_flag()), sums_of(k - 1) if k else None, s)
        acc.sync(s)
        ora.interval(a, L.sizes())
        live.update(L.proc_off, a["proc_slot"], a["node_status"])
        check_tables(acc, ora, live, zones, f"interval {k}")
    acc.export_sums(sums_of(len(plans) - 1), s)
    acc.sync(s)
    e_o, p_o = ora.namespace_totals(off, slots_ns)
    np.testing.assert_array_equal(out_e.cpu().numpy().view(np.uint64), e_o)
    np.testing.assert_array_equal(out_p.cpu().numpy().view(np.uint64), p_o.view(np.uint64))
    assert np.count_nonzero(e_o) > 0
    z = zones
    np.testing.assert_array_equal(out_ne.cpu().numpy().view(np.uint64)[:z],
                                  ora.state["node_active_total"].reshape(-1, z).sum(axis=0, dtype=np.uint64))
    acc.close()
