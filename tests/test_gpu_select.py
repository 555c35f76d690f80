"""kacc_select_above (running workloads above a threshold) — MI355X only.

Whole outputs against tests/select_ref.py (the header's rule in numpy) fed from the oracle's
tables, after each of three intervals of fleets with churn and read errors.  Node sizes cross
every boundary of the kernels (a 64-row mask word, a 256-thread step, the 2048-row tile, several
tiles, empty nodes).  The thresholds come from the oracle's own values over the batch rows, so
the reference decides the share: everything, the median, a value several rows hold, and one above
the largest.  Every output is prefilled with a pattern; what lies at or past min(total, cap)
must still hold it.
"""

import numpy as np
import pytest
import torch

from kepler_amd import accel, fleet
from kepler_amd.torch_batch import current_stream_handle, interval_from_tensors, to_device, top_rows_from_tensors
from oracle.gofmt import joules, label_pairs, sample_line, watts
from oracle.oracle import Oracle
from select_ref import select_above
from top_ref import sort_key

pytestmark = pytest.mark.gpu

KINDS = {"proc": accel.KACC_KIND_PROC, "ctr": accel.KACC_KIND_CTR, "vm": accel.KACC_KIND_VM,
         "pod": accel.KACC_KIND_POD}
ALL_TABLES = [f"{kind}_{what}" for kind in KINDS for what in ("energy", "power")]
SENT64 = 0x5A5A5A5A5A5A5A5A  # output pre-fill: no row, slot, node, energy or power of these tests
SENT32 = 0x5A5A5A5A
NAN_BITS = 0x7FF8000000000000

# name: (node sizes, Z, shuffle_slots)
FLEETS = {
    "edges": ([0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 5000], 4, True),
    "many": ([300, 7, 0, 1000, 64] * 14, 2, False),
    "tiny": ([3], 4, False),
    "z5": ([700, 300, 1300], 5, False),  # odd Z: the 8-byte copy path
    "aligned": ([2048, 0, 2048, 0], 2, True),  # the batch ends on a tile, a node boundary and empty nodes on one
}
CASES = [("edges", t) for t in ALL_TABLES] + [(f, t) for f in ("many", "tiny", "z5")
                                              for t in ("proc_energy", "proc_power", "pod_energy", "pod_power")]


@pytest.fixture(scope="module", autouse=True)
def gpu_ready():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    accel.load()
    torch.cuda.set_stream(torch.cuda.Stream())  # every call below runs on a non-default stream


def make(name, seed=7):
    sizes, zones, shuffle = FLEETS[name]
    L = fleet.make_layout(len(sizes), sizes, zones, seed=seed, shuffle_slots=shuffle, vm_frac=0.05)
    sim = fleet.FleetSim(L, seed=seed, churn=0.05, read_error_frac=0.1)
    return L, sim, accel.Accel(zones, **L.capacities())


class Outputs:
    """Device outputs of one call for `alloc` items, prefilled with the sentinel."""

    def __init__(self, n_nodes, alloc, Z, offset_words=0):
        i32 = lambda m: torch.full((max(m, 1),), SENT32, dtype=torch.int32, device="cuda")  # noqa: E731
        i64 = lambda m: torch.full((max(m, 1),), SENT64, dtype=torch.int64, device="cuda")  # noqa: E731
        self.n_nodes, self.alloc, self.Z = n_nodes, alloc, Z
        self.off, self.row, self.slot, self.node = i32(n_nodes + 1), i32(alloc), i32(alloc), i32(alloc)
        # offset_words = 1: arrays that are 8- but not 16-byte aligned
        self.e_all, self.p_all = i64(alloc * Z + offset_words), i64(alloc * Z + offset_words)
        self.e, self.p = self.e_all[offset_words:], self.p_all[offset_words:]

    def host(self):
        u32 = lambda t, m: t.cpu().numpy().view(np.uint32)[:m]  # noqa: E731
        u64 = lambda t: t.cpu().numpy().view(np.uint64)[: self.alloc * self.Z].reshape(-1, self.Z)  # noqa: E731
        return (u32(self.off, self.n_nodes + 1), u32(self.row, self.alloc), u32(self.slot, self.alloc),
                u32(self.node, self.alloc), u64(self.e), u64(self.p))


def run_select(acc, table, zone, thr, rows, n_nodes, cap, alloc, stream, mask=None, offset_words=0):
    o = Outputs(n_nodes, alloc, acc.zones, offset_words)
    o.mask = torch.from_numpy(np.asarray(mask).astype(np.uint32).view(np.int32)).cuda() if mask is not None else None
    acc.select_above(table, zone, thr, rows, o.mask.data_ptr() if mask is not None else 0, cap, o.off.data_ptr(),
                     o.row.data_ptr(), o.slot.data_ptr(), o.node.data_ptr(), o.e.data_ptr(), o.p.data_ptr(), stream)
    return o


def expect_erange(acc, stream):
    with pytest.raises(accel.AccelError) as e:
        acc.sync(stream)
    assert e.value.code == accel.KACC_ERANGE
    assert "bits 0x1000" in str(e.value) and "4096=select" in str(e.value)


def check(got, want, msg):
    """The first k items and node_off bit for bit; everything past k still the sentinel."""
    k = want[1].shape[0]
    np.testing.assert_array_equal(got[0], want[0], err_msg=f"{msg} node_off")
    for i in range(1, 6):
        assert got[i].dtype == want[i].dtype and got[i].dtype.kind == "u"
        np.testing.assert_array_equal(got[i][:k], want[i], err_msg=f"{msg} output {i}")
        sent = SENT32 if i < 4 else SENT64
        assert np.all(got[i][k:] == sent), f"{msg} output {i} written at or past {k}"


def kind_tables(state, kind):
    return state[f"{kind}_energy"], state[f"{kind}_power"]


def check_caps(acc, state, L, a, t, table, zone, thr, stream, msg, mask=None, caps=None):
    """One threshold at item_cap 0, total - 1, total and total + 7; returns the total."""
    kind, by_power = table.split("_")[0], table.endswith("power")
    energy, power = kind_tables(state, kind)
    ref = lambda cap: select_above(energy, power, L.zones, zone, by_power, a[f"{kind}_off"],  # noqa: E731
                                   a[f"{kind}_slot"], a["node_status"], mask, thr, cap)
    total = int(ref(0)[0][-1])
    rows = top_rows_from_tensors(t, KINDS[kind])
    for cap in (caps or sorted({0, max(total - 1, 0), total, total + 7})):
        o = run_select(acc, table, zone, thr, rows, L.n_nodes, cap, total + 7, stream, mask)
        if 0 < cap < total:
            expect_erange(acc, stream)  # and still the full node_off, checked below
        else:
            acc.sync(stream)  # the sizing call raises nothing
        check(o.host(), ref(cap), f"{msg} cap {cap}/{total}")
    return total


def thresholds(table, zones, zone, a, state):
    """From the oracle's own values over the batch rows: (everything, the median present value, the
    value most rows hold, one above the largest), and how many rows hold the third."""
    kind, by_power = table.split("_")[0], table.endswith("power")
    slots = (a[f"{kind}_slot"] & np.uint32(accel.KACC_SLOT_MASK)).astype(np.int64)
    vals = np.ascontiguousarray(state[table].reshape(-1, zones)[slots, zone])
    bits = vals.view(np.uint64)
    everything = NAN_BITS if by_power else 0
    if bits.size == 0:
        return [everything, everything, everything, 1], 0
    order = np.argsort(sort_key(vals, by_power), kind="stable")
    median = int(bits[order[bits.size // 2]])
    uniq, counts = np.unique(bits, return_counts=True)
    common = int(uniq[np.argmax(counts)])
    if by_power:
        numbers = vals[~np.isnan(vals)]
        above = int(np.nextafter(numbers.max(), np.inf).view(np.uint64)) if numbers.size else 0
    else:
        above = int(bits.max()) + 1
    return [everything, median, common, above], int(counts.max())


@pytest.mark.parametrize("name,table", CASES)
def test_selection_equals_the_rule_over_the_oracle(name, table):
    L, sim, acc = make(name)
    ora = Oracle(L.zones, **L.capacities())
    s = current_stream_handle()
    kind = table.split("_")[0]
    partial, repeated, n_rows = 0, 0, 0
    for it in range(3):
        a = sim.next_interval()
        t = to_device(a)
        acc.run_interval(interval_from_tensors(t, L.sizes()), s)
        ora.interval(a, L.sizes())
        n_rows = a[f"{kind}_slot"].size
        node_of_row = np.repeat(np.arange(L.n_nodes), np.diff(a[f"{kind}_off"].astype(np.int64)))
        listed_rows = int(np.sum((a["node_status"][node_of_row] & accel.KACC_NODE_READ_ERROR) == 0))
        for zone in sorted({0, L.zones - 1}):
            thr, dup = thresholds(table, L.zones, zone, a, ora.state)
            repeated = max(repeated, dup)
            msg = f"{name} {table} it{it} z{zone}"
            assert check_caps(acc, ora.state, L, a, t, table, zone, thr[0], s, msg + " all") == listed_rows
            mid = check_caps(acc, ora.state, L, a, t, table, zone, thr[1], s, msg + " median")
            partial += 0 < mid < listed_rows
            check_caps(acc, ora.state, L, a, t, table, zone, thr[2], s, msg + " repeated")
            assert check_caps(acc, ora.state, L, a, t, table, zone, thr[3], s, msg + " above") == 0
    # over the three intervals together (interval 0 has every power at 0): the median cut a
    # proper share at least once, and some value sat in several rows
    if n_rows > 3:  # the 3-process node has no pod
        assert partial > 0
        assert repeated > 1
    acc.close()


def test_batch_and_nodes_that_end_on_a_tile():
    L, sim, acc = make("aligned", seed=3)
    ora = Oracle(L.zones, **L.capacities())
    s = current_stream_handle()
    for it in range(2):
        a = sim.next_interval()
        t = to_device(a)
        acc.run_interval(interval_from_tensors(t, L.sizes()), s)
        ora.interval(a, L.sizes())
    assert a["proc_off"].tolist() == [0, 2048, 2048, 4096, 4096]
    assert not (a["node_status"][2] & accel.KACC_NODE_READ_ERROR)  # the node behind the boundary is listed
    for table in ("proc_power", "proc_energy"):
        thr, _ = thresholds(table, L.zones, 0, a, ora.state)
        for x in thr:
            check_caps(acc, ora.state, L, a, t, table, 0, x, s, f"aligned {table} thr {x:#x}")
    acc.close()


def test_node_mask_drops_the_unlisted_nodes():
    """Every third node listed, and every third node dropped: the reference with those nodes' rows gone."""
    L, sim, acc = make("many", seed=5)
    ora = Oracle(L.zones, **L.capacities())
    s = current_stream_handle()
    for it in range(2):
        a = sim.next_interval()
        t = to_device(a)
        acc.run_interval(interval_from_tensors(t, L.sizes()), s)
        ora.interval(a, L.sizes())
    third = (np.arange(L.n_nodes) % 3 == 0).astype(np.uint32)
    for table in ("proc_power", "pod_energy"):
        thr, _ = thresholds(table, L.zones, 1, a, ora.state)
        for mask in (third, 1 - third, np.zeros_like(third), third * 0x80000000):
            full = check_caps(acc, ora.state, L, a, t, table, 1, thr[0], s, f"mask {table} all", mask=mask)
            assert (full > 0) == bool(mask.any())
            check_caps(acc, ora.state, L, a, t, table, 1, thr[1], s, f"mask {table} median", mask=mask)
    acc.close()


def test_special_values_follow_the_rule():
    """NaN, negative, -0.0, +Inf and huge ratios in running process slots, the same as stored pod
    powers, and thresholds of every special kind: the rule over the downloaded tables."""
    L, sim, acc = make("edges", seed=11)
    s = current_stream_handle()
    for _ in range(2):
        a = sim.next_interval()
        t = to_device(a)
        acc.run_interval(interval_from_tensors(t, L.sizes()), s)
    acc.sync(s)
    NAN_NEG, NAN_POS = 0xFFF8000000000123, 0x7FF8000000BEEF01  # a NaN keeps its bits in out_power
    special = np.concatenate([np.array([np.nan, -1.5, -0.0, np.inf, 1e300, -np.inf, -1e-300]).view(np.uint64),
                              np.array([NAN_NEG, NAN_POS], dtype=np.uint64)]).view(np.float64)
    rng = np.random.default_rng(3)
    ratio = acc.download("proc_ratio")
    slots = (a["proc_slot"] & np.uint32(accel.KACC_SLOT_MASK)).astype(np.int64)
    pick = rng.choice(slots, size=min(400, slots.size), replace=False)
    ratio[pick] = special[rng.integers(0, special.size, size=pick.size)]
    acc.upload("proc_ratio", ratio)
    Z = L.zones
    pod = acc.download("pod_power").reshape(-1, Z)
    pslots = (a["pod_slot"] & np.uint32(accel.KACC_SLOT_MASK)).astype(np.int64)
    ppick = rng.choice(pslots, size=min(60, pslots.size), replace=False)
    pod[ppick, Z - 1] = special[rng.integers(0, special.size, size=ppick.size)]
    pod[pslots[[0, pslots.size // 2, pslots.size - 1]], Z - 1] = special[[7, 8, 7]]
    acc.upload("pod_power", pod.reshape(-1))
    f64 = lambda x: int(np.array([x], dtype=np.float64).view(np.uint64)[0])  # noqa: E731
    thrs = [NAN_BITS, NAN_NEG, f64(0.0), f64(-0.0), 1, f64(-1.5), f64(-np.inf), f64(np.inf), f64(1e300), f64(-1e-300)]
    for table in ("proc_power", "pod_power"):
        kind = table.split("_")[0]
        state = {f"{kind}_energy": acc.download(f"{kind}_energy"), table: acc.download(table)}
        v = state[table].reshape(-1, Z)[:, Z - 1]
        assert np.isnan(v).any() and (v < 0).any() and np.isinf(v).any() and np.signbit(v[v == 0]).any()
        totals = [check_caps(acc, state, L, a, t, table, Z - 1, thr, s, f"special {table} thr {thr:#x}")
                  for thr in thrs]
        # the consequences the header spells out, on the totals themselves
        assert totals[0] == totals[1] >= totals[6] >= totals[5] >= totals[2] == totals[3] >= totals[4] >= totals[8] >= totals[7] > 0
        assert totals[0] > totals[6]  # the NaNs: below -Inf
        rows = top_rows_from_tensors(t, KINDS[kind])
        o = run_select(acc, table, Z - 1, NAN_BITS, rows, L.n_nodes, totals[0], totals[0], s)
        acc.sync(s)
        got_bits = o.host()[5][:, Z - 1].tolist()
        assert NAN_NEG in got_bits or NAN_POS in got_bits
        assert (1 << 63) in got_bits  # a -0.0 stays -0.0
    acc.close()


@pytest.mark.parametrize("table", ["proc_power", "pod_power", "ctr_energy", "vm_power"])
def test_outputs_are_the_scrape(table):
    """out_energy / out_power equal Accel.download of the kind's tables at out_slot, bit for bit;
    out_row is strictly ascending; out_node agrees with row_off and node_off; 16-byte aligned
    outputs and outputs that are only 8-byte aligned give the same arrays."""
    L, sim, acc = make("edges", seed=5)
    s = current_stream_handle()
    for _ in range(2):
        a = sim.next_interval()
        t = to_device(a)
        acc.run_interval(interval_from_tensors(t, L.sizes()), s)
    acc.sync(s)
    kind, Z = table.split("_")[0], L.zones
    state = {n: acc.download(n) for n in (f"{kind}_energy", f"{kind}_power")}
    thr, _ = thresholds(table, Z, 1, a, state)
    rows = top_rows_from_tensors(t, KINDS[kind])
    n_rows = a[f"{kind}_slot"].size
    for offset_words in (0, 1):
        o = run_select(acc, table, 1, thr[1], rows, L.n_nodes, n_rows, n_rows, s, offset_words=offset_words)
        acc.sync(s)
        off, row, slot, node, e, p = o.host()
        k = int(off[-1])
        assert 0 < k < n_rows
        assert np.all(np.diff(row[:k].astype(np.int64)) > 0)
        np.testing.assert_array_equal(slot[:k], a[f"{kind}_slot"][row[:k]] & np.uint32(accel.KACC_SLOT_MASK))
        roff = a[f"{kind}_off"].astype(np.int64)
        assert np.all((roff[node[:k]] <= row[:k]) & (row[:k] < roff[node[:k] + 1]))
        np.testing.assert_array_equal(np.searchsorted(node[:k], np.arange(L.n_nodes + 1)), off)
        sl = slot[:k].astype(np.int64)
        np.testing.assert_array_equal(e[:k], state[f"{kind}_energy"].reshape(-1, Z)[sl])
        np.testing.assert_array_equal(p[:k], state[f"{kind}_power"].view(np.uint64).reshape(-1, Z)[sl])
        assert np.all(e[k:] == SENT64) and np.all(p[k:] == SENT64)
        assert int(o.e_all[0].item()) == SENT64 and int(o.p_all[0].item()) == SENT64 or offset_words == 0
    acc.close()


def test_single_outputs_and_the_sizing_call():
    """Every output alone (the others NULL) gives the array of the full call."""
    L, sim, acc = make("z5", seed=3)
    s = current_stream_handle()
    for _ in range(2):
        a = sim.next_interval()
        t = to_device(a)
        acc.run_interval(interval_from_tensors(t, L.sizes()), s)
    rows = top_rows_from_tensors(t, accel.KACC_KIND_PROC)
    n_rows = a["proc_slot"].size
    thr = 1  # strictly positive powers
    full = run_select(acc, "proc_power", 0, thr, rows, L.n_nodes, n_rows, n_rows, s)
    acc.sync(s)
    want = full.host()
    assert 0 < int(want[0][-1]) < n_rows
    names = ["row", "slot", "node", "e", "p"]
    for i, name in enumerate(names):
        o = Outputs(L.n_nodes, n_rows, L.zones)
        ptrs = [getattr(o, x).data_ptr() if x == name else 0 for x in names]
        acc.select_above("proc_power", 0, thr, rows, 0, n_rows, o.off.data_ptr(), *ptrs, s)
        acc.sync(s)
        got = o.host()
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[i + 1], want[i + 1])
        for j in range(5):
            if j != i:
                assert np.all(got[j + 1] == (SENT32 if j < 3 else SENT64))
    acc.close()


def test_lines_of_the_selection_byte_exact():
    """Select, then kacc_format_lines_dev on out_energy / out_power with per-item labels: the bytes
    oracle/gofmt.py gives for the same items."""
    L, sim, acc = make("many", seed=9)
    ora = Oracle(L.zones, **L.capacities())
    s = current_stream_handle()
    for _ in range(3):
        a = sim.next_interval()
        t = to_device(a)
        acc.run_interval(interval_from_tensors(t, L.sizes()), s)
        ora.interval(a, L.sizes())
    Z = L.zones
    thr, _ = thresholds("proc_power", Z, 0, a, ora.state)
    rows = top_rows_from_tensors(t, accel.KACC_KIND_PROC)
    want = select_above(ora.state["proc_energy"], ora.state["proc_power"], Z, 0, True, a["proc_off"], a["proc_slot"],
                        a["node_status"], None, thr[1], 2**31)
    T = want[1].shape[0]
    assert 0 < T < a["proc_slot"].size
    o = run_select(acc, "proc_power", 0, thr[1], rows, L.n_nodes, T, T, s)
    labels = [label_pairs([("pid", str(1000 + int(want[2][i]))), ("comm", f"p{int(want[1][i])}"),
                           ("node_name", f"node-{int(want[3][i])}"), ("state", "running")]).encode() for i in range(T)]
    label_off = np.r_[0, np.cumsum([len(x) for x in labels])].astype(np.uint64)
    d_labels = torch.from_numpy(np.frombuffer(b"".join(labels), dtype=np.uint8).copy()).cuda()
    d_loff = torch.from_numpy(label_off.view(np.int64)).cuda()
    zone_names = ["package", "dram"][:Z]
    for is_energy, src, metric, vals in ((True, o.e, "kepler_process_cpu_joules_total", want[4]),
                                         (False, o.p, "kepler_process_cpu_watts", want[5].view(np.float64))):
        d_line_off = torch.zeros(T * Z + 1, dtype=torch.int64, device="cuda")
        args = (is_energy, src.data_ptr(), T, metric, zone_names, d_labels.data_ptr(), d_loff.data_ptr(),
                d_line_off.data_ptr())
        total = acc.format_lines_dev(*args, stream=s)
        out = torch.zeros(total, dtype=torch.uint8, device="cuda")
        assert acc.format_lines_dev(*args, out_ptr=out.data_ptr(), out_cap=total, stream=s) == total
        acc.sync(s)
        text = b"".join(sample_line(metric, labels[i].decode(), zn,
                                    joules(int(vals[i, z])) if is_energy else watts(float(vals[i, z]))).encode()
                        for i in range(T) for z, zn in enumerate(zone_names))
        assert bytes(out.cpu().numpy()) == text
    acc.close()


def test_bad_slot_word_is_left_out_and_reported():
    """A slot word past the capacity: the row is left out, KACC_ERANGE with the select bit, no
    fault; the next correct call on the same context is right."""
    L, sim, acc = make("z5", seed=9)
    ora = Oracle(L.zones, **L.capacities())
    s = current_stream_handle()
    a = sim.next_interval()
    t = to_device(a)
    acc.run_interval(interval_from_tensors(t, L.sizes()), s)
    ora.interval(a, L.sizes())
    acc.sync(s)
    assert (a["node_status"] & accel.KACC_NODE_READ_ERROR).sum() == 0
    bad = dict(t)
    words = a["proc_slot"].copy()
    words[701] = 0xFFFFFFFF
    bad["proc_slot"] = torch.from_numpy(words.view(np.int32)).cuda()
    rows = top_rows_from_tensors(bad, accel.KACC_KIND_PROC)
    n_rows = words.size
    o = run_select(acc, "proc_energy", 0, 0, rows, L.n_nodes, n_rows, n_rows, s)
    expect_erange(acc, s)
    off, row = o.host()[:2]
    assert off.tolist() == [0, 700, 999, n_rows - 1]
    assert row[: n_rows - 1].tolist() == [r for r in range(n_rows) if r != 701] and row[n_rows - 1] == SENT32
    check_caps(acc, ora.state, L, a, t, "proc_energy", 0, 0, s, "after the clamp")
    acc.close()


def test_row_range_outside_the_batch_is_left_out():
    """n_rows short of the last node's range: that node's rows are left out (as a read-error
    node's would be), the others are right, and kacc_sync reports the select bit."""
    L, sim, acc = make("z5", seed=9)
    s = current_stream_handle()
    a = sim.next_interval()
    t = to_device(a)
    acc.run_interval(interval_from_tensors(t, L.sizes()), s)
    acc.sync(s)
    rows = top_rows_from_tensors(t, accel.KACC_KIND_PROC)
    rows.n_rows = 1000  # nodes 0 and 1 own rows [0, 1000)
    want = select_above(acc.download("proc_energy"), acc.download("proc_power"), L.zones, 1, False, a["proc_off"],
                        a["proc_slot"], np.array([0, 0, accel.KACC_NODE_READ_ERROR], dtype=np.uint32), None, 0, 2300)
    assert want[0].tolist() == [0, 700, 1000, 1000]
    o = run_select(acc, "proc_energy", 1, 0, rows, L.n_nodes, 2300, 2300, s)
    expect_erange(acc, s)
    check(o.host(), want, "short n_rows")
    acc.close()


def test_host_errors_launch_nothing():
    L, sim, acc = make("tiny")
    s = current_stream_handle()
    a = sim.next_interval()
    t = to_device(a)
    acc.run_interval(interval_from_tensors(t, L.sizes()), s)
    rows = top_rows_from_tensors(t, accel.KACC_KIND_PROC)
    o = Outputs(L.n_nodes, 8, L.zones)
    outs = [o.row.data_ptr(), o.slot.data_ptr(), o.node.data_ptr(), o.e.data_ptr(), o.p.data_ptr()]
    lib, ctx, T = acc.lib, acc.ctx, accel.TABLE_INDEX

    def call(table=T["proc_power"], zone=0, r=rows, cap=8, off=o.off.data_ptr(), out=outs, c=ctx):
        return lib.kacc_select_above(c, table, zone, 0, r, None, cap, off, *out, s)

    no_off, no_slot, many = (accel.KaccTopRows() for _ in range(3))
    for r in (no_off, no_slot, many):
        r.n_nodes, r.n_rows, r.row_off, r.slot, r.node_status = (rows.n_nodes, rows.n_rows, rows.row_off, rows.slot,
                                                                 rows.node_status)
    no_off.row_off = None
    no_slot.slot = None
    many.n_nodes = L.n_nodes + 1
    assert call(c=None) == accel.KACC_EINVAL
    assert call(r=None) == accel.KACC_EINVAL
    assert call(r=no_off) == accel.KACC_EINVAL
    assert call(r=no_slot) == accel.KACC_EINVAL
    assert call(off=None) == accel.KACC_EINVAL
    assert call(table=T["node_power"]) == accel.KACC_EINVAL
    assert call(table=T["proc_ratio"]) == accel.KACC_EINVAL
    assert call(table=len(accel.TABLES)) == accel.KACC_EINVAL  # KACC_T_COUNT
    assert call(zone=L.zones) == accel.KACC_EINVAL
    assert call(r=many) == accel.KACC_EINVAL
    assert call(out=[None] * 5) == accel.KACC_EINVAL
    assert call(table=T["proc_energy"], cap=0, out=[None] * 5) == accel.KACC_OK  # the sizing call needs no output
    acc.sync(s)  # nothing raised
    listed = not (int(a["node_status"][0]) & accel.KACC_NODE_READ_ERROR)
    assert o.off.cpu().numpy().view(np.uint32).tolist() == [0, 3 if listed else 0]
    # a batch without nodes is no error: node_off[0] = 0 and nothing else
    none = accel.KaccTopRows()
    none.n_nodes, none.n_rows, none.row_off, none.slot, none.node_status = 0, 0, rows.row_off, None, None
    o.off.fill_(SENT32)
    assert call(r=none) == accel.KACC_OK
    acc.sync(s)
    assert o.off.cpu().numpy().view(np.uint32).tolist() == [0, SENT32]
    for x in (o.row, o.slot, o.node):
        assert np.all(x.cpu().numpy().view(np.uint32) == SENT32)
    acc.close()


def test_second_stream_gives_the_same_selection():
    """The interval and the call on a second, non-default stream; the next interval behind it."""
    results = []
    for two in (False, True):
        L, sim, acc = make("many", seed=13)
        st = torch.cuda.Stream() if two else torch.cuda.current_stream()
        got = []
        with torch.cuda.stream(st):
            for _ in range(3):
                a = sim.next_interval()
                t = to_device(a)
                n_rows = a["proc_slot"].size
                acc.run_interval(interval_from_tensors(t, L.sizes()), st.cuda_stream)
                rows = top_rows_from_tensors(t, accel.KACC_KIND_PROC)
                got.append((run_select(acc, "proc_power", 0, 1, rows, L.n_nodes, n_rows, n_rows, st.cuda_stream), t))
            acc.sync(st.cuda_stream)
        results.append([o.host() for o, _ in got])
        acc.close()
    for one, other in zip(*results):
        for x, y in zip(one, other):
            np.testing.assert_array_equal(x, y)
    assert 0 < int(results[0][-1][0][-1])
