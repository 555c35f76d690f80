"""Terminated workloads exported on the device (kacc_tracker_read + kacc_format_lines_dev) — MI355X only.

The reference writes every workload family twice per scrape
(power_collector.go:225-243): the running set with state="running" and the
terminated trackers' items with state="terminated".  kacc_tracker_read is
Items() on the device (asynchronous, per node mask, optionally clearing);
kacc_format_lines_dev writes the sample lines of its dense outputs.

Trackers are filled as tests/test_gpu_tracker.py fills them: acc.upload of the
kind's tables, a SlotMap for slot_off, hand-made term_* arrays, Tracker.add.
Within every node the target-zone energies are pairwise distinct, so a node's
order is fully determined and the read must equal Tracker.items() bit for bit.
"""

import hashlib
import json
import os

import numpy as np
import pytest
import torch

from kepler_amd import accel
from kepler_amd.torch_batch import current_stream_handle
from oracle.gofmt import joules, label_pairs, sample_line, watts

pytestmark = pytest.mark.gpu

KINDS = {"proc": accel.KACC_KIND_PROC, "ctr": accel.KACC_KIND_CTR, "vm": accel.KACC_KIND_VM,
         "pod": accel.KACC_KIND_POD}
SENT64 = 0x5A5A5A5A5A5A5A5A  # output pre-fill: no key, energy or power bit pattern of these tests
SENT32 = 0x5A5A5A5A
ZONE = 1  # the trackers' target zone
ALPHABET = ['a', 'Z', '0', '/', '-', '"', '\\', '\n', 'é', ' ', '{', '=']  # test_format_lines_byte_exact's


@pytest.fixture(scope="module", autouse=True)
def gpu_ready():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    accel.load()
    torch.cuda.set_stream(torch.cuda.Stream())  # every call below runs on a non-default stream


def shape_a_sizes():
    """Shape A: 70 nodes (more than one wave of nodes), candidates per node for max_size 5:
    0, 1, max_size, more than max_size (8 -> 5 kept), and runs of empty nodes at the start,
    in the middle and at the end."""
    s = np.random.default_rng(5).integers(0, 6, size=70)
    s[:3] = 0
    s[3], s[4], s[5] = 1, 5, 8
    s[30:35] = 0
    s[35] = 5
    s[-4:] = 0
    return s


def shape_b_sizes():
    """Shape B: counts that cross a wave (65) and a 256-thread workgroup (257), one item, a full
    node (300 = capacity); the rest empty."""
    s = np.zeros(12, dtype=np.int64)
    s[1], s[4], s[7], s[10] = 1, 65, 257, 300
    return s


class Filled:
    """A tracker of one kind over len(cand) nodes after ONE add of cand[n] terminated workloads
    per node (queued on the current stream, not synchronized)."""

    def __init__(self, kind, Z, cand, max_size, capacity=0, seed=1, edit=None):
        cand = np.asarray(cand, dtype=np.int64)
        self.kind, self.Z, self.N = kind, Z, cand.size
        slot_off = np.r_[0, np.cumsum(np.maximum(cand, 1))].astype(np.uint32)
        S = int(slot_off[-1])
        caps = {f"{k}_slots": 1 for k in KINDS}
        caps[f"{kind}_slots"] = S
        self.acc = acc = accel.Accel(Z, nodes=self.N, **caps)
        rng = np.random.default_rng(seed)
        node_of = np.repeat(np.arange(self.N), np.diff(slot_off.astype(np.int64)))
        e = rng.integers(1, 2**40, size=(S, Z), dtype=np.uint64)
        e[:, ZONE] = 10**6 + rng.permutation(S).astype(np.uint64) * 3  # pairwise distinct
        p = rng.random((S, Z)) * 10.0 ** rng.integers(-3, 9, size=(S, Z))
        ratio = rng.random(S)
        keep = max_size if max_size > 0 else capacity
        if edit:  # slots that are added and all kept (their node has no more candidates than it keeps)
            rank = np.arange(S) - slot_off[node_of].astype(np.int64)
            edit(e, p, ratio, np.flatnonzero((rank < cand[node_of]) & (cand[node_of] <= keep)))
        acc.upload(f"{kind}_energy", e.reshape(-1))
        if kind == "pod":  # the power is the stored record
            acc.upload("pod_power", p.reshape(-1))
        else:  # derived: ratio x the node's ActivePower, behind the guard (process.go:124)
            acc.upload(f"{kind}_ratio", ratio)
            acc.upload(f"{kind}_node", node_of.astype(np.uint32))
            acc.upload("node_active_power", np.ones(self.N * Z) if edit else rng.random(self.N * Z) * 1e8 + 1.0)
            acc.upload("node_active_energy", np.ones(self.N * Z, dtype=np.uint64))
            acc.upload("node_cpu_delta", np.ones(self.N))
        self.sm = accel.SlotMap(acc, KINDS[kind], slot_off)
        self.tr = accel.Tracker(acc, KINDS[kind], max_size, zone=ZONE, min_energy=0, capacity=capacity)
        # node n's terminated segment: its first cand[n] slots, keys 1000 + slot
        self.tk = torch.from_numpy(1000 + np.arange(S, dtype=np.int64)).cuda()
        self.ts = torch.from_numpy(np.arange(S, dtype=np.int32)).cuda()
        self.tc = torch.from_numpy(cand.astype(np.int32)).cuda()
        self.sizes = np.minimum(cand, keep)
        self.total = int(self.sizes.sum())
        self.s = current_stream_handle()
        self.tr.add(self.sm, self.tk.data_ptr(), self.ts.data_ptr(), self.tc.data_ptr(), self.s)

    def read(self, item_cap, alloc=None, mask=None, flags=0, sync=True):
        """Tracker.read into sentinel-filled device arrays of `alloc` items; returns host copies
        (off u32[N + 1], key u64, node u32, energy u64 [alloc, Z], power BITS u64 [alloc, Z]) and
        keeps the device tensors in self.dev."""
        alloc = item_cap if alloc is None else alloc
        Z = self.Z
        d_off = torch.full((self.N + 1,), SENT32, dtype=torch.int32, device="cuda")
        d_key = torch.full((max(alloc, 1),), SENT64, dtype=torch.int64, device="cuda")
        d_node = torch.full((max(alloc, 1),), SENT32, dtype=torch.int32, device="cuda")
        d_e = torch.full((max(alloc, 1) * Z,), SENT64, dtype=torch.int64, device="cuda")
        d_p = torch.full((max(alloc, 1) * Z,), SENT64, dtype=torch.int64, device="cuda")
        d_mask = (torch.from_numpy(np.asarray(mask).astype(np.uint32).view(np.int32)).cuda()
                  if mask is not None else None)
        self.tr.read(d_off.data_ptr(), item_cap, d_key.data_ptr(), d_node.data_ptr(), d_e.data_ptr(),
                     d_p.data_ptr(), node_mask_ptr=d_mask.data_ptr() if mask is not None else 0, flags=flags,
                     stream=self.s)
        self.dev = (d_off, d_key, d_node, d_e, d_p, d_mask)
        if sync:
            self.acc.sync(self.s)
        return self.host()

    def host(self):
        d_off, d_key, d_node, d_e, d_p, _ = self.dev
        return (d_off.cpu().numpy().view(np.uint32), d_key.cpu().numpy().view(np.uint64),
                d_node.cpu().numpy().view(np.uint32), d_e.cpu().numpy().view(np.uint64).reshape(-1, self.Z),
                d_p.cpu().numpy().view(np.uint64).reshape(-1, self.Z))

    def items(self):
        k, nd, e, p = self.tr.items()
        return k.copy(), nd.copy(), e.copy(), p.view(np.uint64).copy()


def check_read(got, want, sizes_listed, count=None, alloc_tail=True):
    """got (a read's host copies) == want (items(), filtered) in the first `count` items, bit for
    bit; node_off = the cumulative sizes; everything at and past `count` still the sentinel."""
    off, k, nd, e, p = got
    wk, wn, we, wp = want
    total = int(np.sum(sizes_listed))
    assert wk.size == total
    np.testing.assert_array_equal(off, np.r_[0, np.cumsum(sizes_listed)].astype(np.uint32))
    c = total if count is None else count
    np.testing.assert_array_equal(k[:c], wk[:c])
    np.testing.assert_array_equal(nd[:c], wn[:c])
    np.testing.assert_array_equal(e[:c], we[:c])
    np.testing.assert_array_equal(p[:c], wp[:c])  # power as bits
    if alloc_tail:
        assert np.all(k[c:] == SENT64) and np.all(nd[c:] == SENT32)
        assert np.all(e[c:] == SENT64) and np.all(p[c:] == SENT64)


def check_order(got, total):
    """Independently of items(): out_node non-decreasing, each node's target-zone energies
    strictly descending."""
    _, _, nd, e, _ = got
    nd, ez = nd[:total].astype(np.int64), e[:total, ZONE]
    assert np.all(np.diff(nd) >= 0)
    same = np.diff(nd) == 0
    assert np.all(ez[1:][same] < ez[:-1][same])


def filtered(want, mask):
    keep = np.asarray(mask)[want[1]] != 0
    return tuple(a[keep] for a in want)


SHAPES = [
    ("A-z3", "proc", 3, shape_a_sizes, 5, 0),
    ("A-z4", "proc", 4, shape_a_sizes, 5, 0),
    ("B-pod-unlimited", "pod", 4, shape_b_sizes, -1, 300),
]


@pytest.mark.parametrize("name,kind,Z,sizes,max_size,capacity", SHAPES, ids=[s[0] for s in SHAPES])
def test_read_equals_items(name, kind, Z, sizes, max_size, capacity):
    """1. Tracker.read on a non-default stream, queued behind the add with no host sync between
    them, is Tracker.items() bit for bit; the outputs hold 8 more items than the total."""
    f = Filled(kind, Z, sizes(), max_size, capacity)
    got = f.read(f.total + 8)  # add -> read on one stream; the sync comes after the read
    if name.startswith("A"):
        assert {0, 1, max_size} <= set(f.sizes.tolist())
    else:
        assert sorted(f.sizes[f.sizes > 0].tolist()) == [1, 65, 257, 300]
    check_read(got, f.items(), f.sizes)
    check_order(got, f.total)
    f.acc.close()


def test_read_into_8_byte_aligned_outputs():
    """Z = 4 outputs that are only 8-byte aligned (the 16-byte copies do not apply): the same
    items, and the words around the outputs untouched."""
    f = Filled("proc", 4, shape_a_sizes(), 5)
    T, Z = f.total, 4
    d_off = torch.zeros(f.N + 1, dtype=torch.int32, device="cuda")
    d_e = torch.full((T * Z + 2,), SENT64, dtype=torch.int64, device="cuda")
    d_p = torch.full((T * Z + 2,), SENT64, dtype=torch.int64, device="cuda")
    assert d_e.data_ptr() % 16 == 0 and d_p.data_ptr() % 16 == 0
    f.tr.read(d_off.data_ptr(), T, out_energy_ptr=d_e.data_ptr() + 8, out_power_ptr=d_p.data_ptr() + 8, stream=f.s)
    f.acc.sync(f.s)
    _, _, we, wp = f.items()
    for d, w in ((d_e, we), (d_p, wp)):
        h = d.cpu().numpy().view(np.uint64)
        assert h[0] == SENT64 and h[-1] == SENT64
        np.testing.assert_array_equal(h[1:-1].reshape(-1, Z), w)
    f.acc.close()


def test_mask_and_clear():
    """2. Masks (every third node, none, NULL) and KACC_TRACKER_READ_CLEAR on shape A."""
    f = Filled("proc", 4, shape_a_sizes(), 5)
    third = (np.arange(f.N) % 3 == 0).astype(np.int32)
    first = f.read(f.total + 8)
    want = f.items()
    check_read(first, want, f.sizes)
    for mask in (third, np.zeros(f.N, dtype=np.int32)):
        got = f.read(f.total + 8, mask=mask)
        check_read(got, filtered(want, mask), f.sizes * (mask != 0))
    assert f.read(f.total + 8, mask=np.zeros(f.N, dtype=np.int32))[0][-1] == 0
    # a nonzero mask entry of any value lists the node
    check_read(f.read(f.total + 8, mask=third.astype(np.int64) * 0x80000000), filtered(want, third),
               f.sizes * third)
    # read + clear of the listed nodes: the others keep their items, unchanged
    got = f.read(f.total + 8, mask=third, flags=accel.KACC_TRACKER_READ_CLEAR)
    check_read(got, filtered(want, third), f.sizes * third)
    rest = f.items()
    for a, b in zip(rest, filtered(want, 1 - third)):
        np.testing.assert_array_equal(a, b)
    again = f.read(f.total + 8, mask=third)
    assert again[0][-1] == 0 and np.all(again[0] == 0) and np.all(again[1] == SENT64)
    # NULL mask + clear empties every node
    check_read(f.read(f.total + 8, flags=accel.KACC_TRACKER_READ_CLEAR), rest, f.sizes * (1 - third))
    assert f.items()[0].size == 0
    f.acc.close()


def test_scan_across_tiles():
    """3. 5,000 nodes of 0, 1 or 2 items: the offsets' scan (5,001 values) crosses the boundary
    of its 4,096-value tile."""
    cand = np.random.default_rng(9).integers(0, 3, size=5000)
    f = Filled("proc", 4, cand, 2)
    got = f.read(f.total + 8)
    assert f.total > 4096 and set(f.sizes.tolist()) == {0, 1, 2}
    check_read(got, f.items(), f.sizes)
    check_order(got, f.total)
    f.acc.close()


def test_short_capacity():
    """4. item_cap = total - 3: KACC_ERANGE at kacc_sync naming the tracker read, items
    [0, item_cap) correct, an 8-item guard behind item_cap intact, node_off the full offsets;
    with READ_CLEAR nothing is cleared; the sizing call writes only node_off."""
    f = Filled("proc", 4, shape_a_sizes(), 5)
    cap = f.total - 3
    f.read(cap, alloc=cap + 8, sync=False)
    with pytest.raises(accel.AccelError, match="tracker read") as ei:
        f.acc.sync(f.s)
    assert ei.value.code == accel.KACC_ERANGE and "bits 0x800:" in str(ei.value)  # that bit alone
    got, want = f.host(), f.items()
    check_read(got, want, f.sizes, count=cap)
    assert got[1].size == cap + 8  # the guard check_read saw
    f.read(cap, alloc=cap + 8, flags=accel.KACC_TRACKER_READ_CLEAR, sync=False)
    with pytest.raises(accel.AccelError, match="tracker read"):
        f.acc.sync(f.s)
    check_read(f.host(), want, f.sizes, count=cap)
    for a, b in zip(f.items(), want):  # nothing was cleared
        np.testing.assert_array_equal(a, b)
    # sizing: item_cap 0, every output NULL
    d_off = torch.full((f.N + 1,), SENT32, dtype=torch.int32, device="cuda")
    f.tr.read(d_off.data_ptr(), 0, stream=f.s)
    f.acc.sync(f.s)  # no error: a sizing call is not a short read
    np.testing.assert_array_equal(d_off.cpu().numpy().view(np.uint32), np.r_[0, np.cumsum(f.sizes)])
    # bad arguments launch nothing
    with pytest.raises(accel.AccelError):
        f.tr.read(d_off.data_ptr(), 4, stream=f.s)  # item_cap > 0, all outputs NULL
    with pytest.raises(accel.AccelError):
        f.tr.read(d_off.data_ptr(), 0, flags=0x2, stream=f.s)  # unknown flag
    f.acc.sync(f.s)
    f.acc.close()


def test_disabled_tracker_reads_empty():
    acc = accel.Accel(2, nodes=3, proc_slots=1, ctr_slots=1, vm_slots=1, pod_slots=1)
    tr = accel.Tracker(acc, accel.KACC_KIND_PROC, 0, zone=0, min_energy=0)
    d_off = torch.full((4,), SENT32, dtype=torch.int32, device="cuda")
    d_key = torch.full((4,), SENT64, dtype=torch.int64, device="cuda")
    s = current_stream_handle()
    tr.read(d_off.data_ptr(), 4, d_key.data_ptr(), stream=s)
    acc.sync(s)
    assert np.all(d_off.cpu().numpy() == 0) and np.all(d_key.cpu().numpy() == SENT64)
    acc.close()


def _special_values(kind):
    def edit(e, p, ratio, kept):
        Z = e.shape[1]
        other = [z for z in range(Z) if z != ZONE]  # the target zone keeps its distinct energies
        for i, v in enumerate([0, 1, 10**6, 2**64 - 1]):  # frozen energies
            e[kept[(7 * i + 3) % kept.size], other[i % len(other)]] = v
        specials = [0.0, -0.0, float("nan"), float("inf"), 1e-300]
        for i, v in enumerate(specials):
            p[kept[(5 * i + 1) % kept.size], i % Z] = v  # pods: the stored record
            ratio[kept[(5 * i + 1) % kept.size]] = v  # others: ratio x ActivePower 1.0
    return edit


@pytest.mark.parametrize("kind", ["proc", "pod"])
def test_lines_byte_exact(kind):
    """5. kacc_format_lines_dev over a read's out_energy / out_power: byte for byte
    oracle/gofmt.sample_line, per-item labels with state="terminated", a zone subset in a
    caller-chosen order, a row permutation, a sizing call first, a short out_cap raising; the
    same dense arrays uploaded into tables give the identical bytes through
    kacc_format_lines.  "proc" is shape A as it stands (the power derived: special powers come
    from special ratios x an ActivePower of 1.0); "pod" is shape A's sizes with the pod kind,
    whose power is the stored record, so the special powers are uploaded as they are."""
    Z = 4
    f = Filled(kind, Z, shape_a_sizes(), 5, edit=_special_values(kind))
    off, keys, nodes, e, p_bits = f.read(f.total)
    T = f.total
    check_read((off, keys, nodes, e, p_bits), f.items(), f.sizes)
    p = p_bits.view(np.float64)
    assert {0, 1, 10**6, 2**64 - 1} <= set(e.reshape(-1).tolist())
    assert np.isnan(p).any() and np.isinf(p).any() and (p == 1e-300).any()
    assert np.any((p == 0) & np.signbit(p)) and np.any((p == 0) & ~np.signbit(p))
    d_e, d_p = f.dev[3], f.dev[4]
    rng = np.random.default_rng(17)
    rows = []
    for i in range(T):
        comm = "".join(rng.choice(ALPHABET, size=int(rng.integers(0, 12))))
        rows.append(label_pairs([("pid", str(int(keys[i]))), ("comm", comm), ("container_id", ""),
                                 ("exe", "/usr/bin/" + comm), ("node_name", f"node-{int(nodes[i])}"),
                                 ("state", "terminated"), ("type", "regular"), ("vm_id", "")]).encode())
    label_off = np.r_[0, np.cumsum([len(x) for x in rows])].astype(np.uint64)
    d_labels = torch.from_numpy(np.frombuffer(b"".join(rows), dtype=np.uint8).copy()).cuda()
    d_loff = torch.from_numpy(label_off.view(np.int64)).cuda()
    order = rng.permutation(T).astype(np.uint32)
    d_order = torch.from_numpy(order.view(np.int32)).cuda()
    zone_order, zone_names = [3, 0, 2], ["dram", "package", "uncore"]
    n_lines = T * len(zone_order)
    # the same arrays as table rows (pod_power is a stored table)
    ref = accel.Accel(Z, nodes=1, proc_slots=T, ctr_slots=1, vm_slots=1, pod_slots=T)
    ref.upload("proc_energy", e.reshape(-1))
    ref.upload("pod_power", p.reshape(-1))
    s = f.s
    for is_energy, src, metric, table in ((True, d_e, "kepler_process_cpu_joules_total", "proc_energy"),
                                          (False, d_p, "kepler_process_cpu_watts", "pod_power")):
        d_line_off = torch.zeros(n_lines + 1, dtype=torch.int64, device="cuda")
        args = (is_energy, src.data_ptr(), T, metric, zone_names, d_labels.data_ptr(), d_loff.data_ptr(),
                d_line_off.data_ptr())
        kw = dict(zone_order=zone_order, row_order_ptr=d_order.data_ptr(), stream=s)
        total = f.acc.format_lines_dev(*args, **kw)  # sizing call
        with pytest.raises(accel.AccelError) as ei:  # too small a buffer: KACC_ERANGE
            small = torch.zeros(16, dtype=torch.uint8, device="cuda")
            f.acc.format_lines_dev(*args, out_ptr=small.data_ptr(), out_cap=16, **kw)
        assert ei.value.code == accel.KACC_ERANGE
        out = torch.zeros(total, dtype=torch.uint8, device="cuda")
        assert f.acc.format_lines_dev(*args, out_ptr=out.data_ptr(), out_cap=total, **kw) == total
        f.acc.sync(s)
        got = bytes(out.cpu().numpy())
        offs = d_line_off.cpu().numpy()
        assert offs[0] == 0 and offs[-1] == total and np.all(np.diff(offs) > 0)
        li = 0
        for i in range(T):
            r = int(order[i])
            for z, zn in zip(zone_order, zone_names):
                v = joules(int(e[r, z])) if is_energy else watts(float(p[r, z]))
                want = sample_line(metric, rows[r].decode(), zn, v).encode()
                assert got[offs[li]:offs[li + 1]] == want, (i, r, z)
                li += 1
        # cross-check: the table path over the same values
        t_off = torch.zeros(n_lines + 1, dtype=torch.int64, device="cuda")
        targs = (table, metric, 0, T, zone_names, d_labels.data_ptr(), d_loff.data_ptr(), t_off.data_ptr())
        assert ref.format_lines(*targs, **kw) == total
        t_out = torch.zeros(total, dtype=torch.uint8, device="cuda")
        ref.format_lines(*targs, out_ptr=t_out.data_ptr(), out_cap=total, **kw)
        ref.sync(s)
        assert bytes(t_out.cpu().numpy()) == got
        assert torch.equal(t_off, d_line_off)
    ref.close()
    f.acc.close()


def _parse_exposition(text):
    """Sample lines of the text format -> [(name, {label: value}, float)] (label values
    unescaped: \\\\, \\" and \\n, expfmt's escapes), as tests/test_gpu_format.py parses them."""
    out = []
    for line in text.splitlines():
        name, rest = line.split("{", 1)
        labels, i = {}, 0
        while rest[i] != "}":
            eq = rest.index("=", i)
            key = rest[i:eq]
            assert rest[eq + 1] == '"', line
            j, val = eq + 2, []
            while rest[j] != '"':
                if rest[j] == "\\":
                    val.append({"\\": "\\", '"': '"', "n": "\n"}[rest[j + 1]])
                    j += 2
                else:
                    val.append(rest[j])
                    j += 1
            labels[key] = "".join(val)
            i = j + 1
            if rest[i] == ",":
                i += 1
        assert rest[i + 1] == " ", line
        out.append((name, labels, float(rest[i + 2:])))
    return out


FIXTURE = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "terminated_export.json")))


def _key_of(kind, labels, id_label):
    if kind == "proc":
        return int(labels[id_label])  # the PID
    return int.from_bytes(hashlib.sha256(labels[id_label].encode()).digest()[:8], "little") >> 1


@pytest.mark.parametrize("fam,kind", [("process", "proc"), ("container", "ctr"), ("vm", "vm")])
def test_reference_terminated_export(fam, kind):
    """6. TestTerminatedProcessExport / ContainerExport / VMExport
    (power_collector_test.go:513-615, 865-960, 962-1058; tests/golden/terminated_export.json), one
    node, one zone.  The running workload is held in the tables and written by
    kacc_format_lines; the terminated one takes the real path: present in one kacc_slot_join,
    its final energy and ratio uploaded, absent in the next join, then Tracker.add ->
    Tracker.read (clearing) -> kacc_format_lines_dev.  The joined text, parsed back, satisfies
    every assertion of the reference test; every device line also equals sample_line."""
    fx = FIXTURE["kinds"][fam]
    zone, node_name = FIXTURE["zone"]["name"], FIXTURE["node_name"]
    run, term = fx["running"], fx["terminated"]
    caps = {f"{k}_slots": 1 for k in KINDS}
    caps[f"{kind}_slots"] = 2
    acc = accel.Accel(1, nodes=1, **caps)
    sm = accel.SlotMap(acc, KINDS[kind], np.array([0, 2], dtype=np.uint32))
    tr = accel.Tracker(acc, KINDS[kind], 500, zone=0, min_energy=0)
    s = current_stream_handle()
    kdt = np.uint32 if kind == "proc" else np.uint64
    k_run, k_term = _key_of(kind, run["labels"], fx["id_label"]), _key_of(kind, term["labels"], fx["id_label"])
    tk = torch.zeros(2, dtype=torch.int64, device="cuda")
    ts = torch.zeros(2, dtype=torch.int32, device="cuda")
    tc = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_slot = torch.zeros(2, dtype=torch.int32, device="cuda")

    def join(keys):
        d_keys = torch.from_numpy(np.array(keys, dtype=kdt).view(np.uint8)).cuda()
        d_off = torch.tensor([0, len(keys)], dtype=torch.int32, device="cuda")
        sm.join(len(keys), d_off.data_ptr(), d_keys.data_ptr(), 0, d_slot.data_ptr(), tk.data_ptr(), ts.data_ptr(),
                tc.data_ptr(), s)
        acc.sync(s)
        return [int(x) & accel.KACC_SLOT_MASK for x in d_slot.cpu().numpy().view(np.uint32)[:len(keys)]]

    slot_run, slot_term = join([k_run, k_term])  # both alive
    assert int(tc.item()) == 0
    # the interval's results: ActivePower 10 W (the node's Power; no idle share), so the
    # derived power ratio x ActivePower is exact; the derive guard's other operands nonzero
    active = float(FIXTURE["node"]["power"])
    acc.upload("node_active_power", np.array([active]))
    acc.upload("node_active_energy", np.array([FIXTURE["node"]["energy_total"]], dtype=np.uint64))
    acc.upload("node_cpu_delta", np.array([1.0]))
    for w, slot in ((run, slot_run), (term, slot_term)):
        acc.upload(f"{kind}_energy", np.array([w["energy_total"]], dtype=np.uint64), slot)
        acc.upload(f"{kind}_ratio", np.array([w["power"] / active]), slot)
        acc.upload(f"{kind}_node", np.array([0], dtype=np.uint32), slot)
    assert join([k_run]) == [slot_run]  # the second workload is gone
    assert int(tc.item()) == 1
    # terminated half of the scrape: add -> read + clear -> keys back -> labels -> lines
    tr.add(sm, tk.data_ptr(), ts.data_ptr(), tc.data_ptr(), s)
    d_noff = torch.zeros(2, dtype=torch.int32, device="cuda")
    d_key = torch.zeros(4, dtype=torch.int64, device="cuda")
    d_node = torch.zeros(4, dtype=torch.int32, device="cuda")
    d_e = torch.zeros(4, dtype=torch.int64, device="cuda")
    d_p = torch.zeros(4, dtype=torch.float64, device="cuda")
    tr.read(d_noff.data_ptr(), 4, d_key.data_ptr(), d_node.data_ptr(), d_e.data_ptr(), d_p.data_ptr(),
            flags=accel.KACC_TRACKER_READ_CLEAR, stream=s)
    acc.sync(s)
    assert d_noff.cpu().tolist() == [0, 1] and int(d_key[0].item()) == k_term and int(d_node[0].item()) == 0
    assert tr.items()[0].size == 0  # Clear() after the export (process.go:80-84)

    def labels_of(w, state):
        return label_pairs(list(w["labels"].items()) + [("state", state), ("node_name", node_name)])

    def run_lines(call, lab):
        d_labels = torch.from_numpy(np.frombuffer(lab.encode(), np.uint8).copy()).cuda()
        d_loff = torch.tensor([0, len(lab.encode())], dtype=torch.int64, device="cuda")
        d_line_off = torch.zeros(2, dtype=torch.int64, device="cuda")
        total = call(d_labels.data_ptr(), d_loff.data_ptr(), d_line_off.data_ptr(), 0, 0)
        out = torch.zeros(total, dtype=torch.uint8, device="cuda")
        call(d_labels.data_ptr(), d_loff.data_ptr(), d_line_off.data_ptr(), out.data_ptr(), total)
        acc.sync(s)
        return bytes(out.cpu().numpy()).decode()

    text, want = [], []
    for metric, is_energy in zip(fx["metrics"], (True, False)):
        table = f"{kind}_energy" if is_energy else f"{kind}_power"
        lab = labels_of(run, "running")
        text.append(run_lines(lambda lp, lo, lf, o, c: acc.format_lines(
            table, metric, slot_run, 1, [zone], lp, lo, lf, out_ptr=o, out_cap=c, stream=s), lab))
        want.append(sample_line(metric, lab, zone,
                                joules(run["energy_total"]) if is_energy else watts(float(run["power"]))))
        lab = labels_of(term, "terminated")
        src = d_e if is_energy else d_p
        text.append(run_lines(lambda lp, lo, lf, o, c: acc.format_lines_dev(
            is_energy, src.data_ptr(), 1, metric, [zone], lp, lo, lf, out_ptr=o, out_cap=c, stream=s), lab))
        want.append(sample_line(metric, lab, zone,
                                joules(term["energy_total"]) if is_energy else watts(float(term["power"]))))
    assert text == want  # byte-exact against the restated expfmt
    samples = _parse_exposition("".join(text))
    for chk in fx["checks"]:  # assertMetricLabelValues
        hits = [val for n, lb, val in samples
                if n == chk["metric"] and all(lb.get(k) == x for k, x in chk["labels"].items())]
        assert hits == [chk["value"]], chk
    for chk in fx["exists"]:  # assertMetricExists
        assert any(n == chk["metric"] and all(lb.get(k) == x for k, x in chk["labels"].items())
                   for n, lb, _ in samples), chk
    assert all(lb["node_name"] == node_name and lb["zone"] == zone for _, lb, _ in samples)
    acc.close()
