"""kacc_group_sums (running workloads summed by a caller-defined group) — MI355X only.

Whole outputs, bit for bit, against tests/group_ref.py (the header's contract in numpy) fed from
the oracle's tables, after each of three intervals of fleets with churn and read errors.  Node
sizes cross every boundary of the kernel (a 64-row word, a 256-thread step, the 2048-row tile,
several tiles, empty nodes, a batch that ends on a tile); the group counts cross every bin
capacity (replicated bins, one copy, one pass, several passes); the group ids come in four
patterns, each with about 5 % KACC_GROUP_NONE.  Every output is prefilled with a pattern, so a
word the call did not write shows.  No tolerance anywhere: every sum is an integer.
"""

import numpy as np
import pytest
import torch

from group_ref import fx, group_sums
from kepler_amd import accel, fleet
from kepler_amd.torch_batch import current_stream_handle, interval_from_tensors, to_device, top_rows_from_tensors
from oracle.gofmt import label_pairs, sample_line, watts
from oracle.oracle import Oracle
from plan_ref import group_regime  # kacc_group.hip's LDS plan, restated

pytestmark = pytest.mark.gpu

KINDS = {"proc": accel.KACC_KIND_PROC, "ctr": accel.KACC_KIND_CTR, "vm": accel.KACC_KIND_VM,
         "pod": accel.KACC_KIND_POD}
NONE = accel.KACC_GROUP_NONE
SENT64 = 0x5A5A5A5A5A5A5A5A  # output pre-fill
SENT32 = 0x5A5A5A5A
N_GROUPS = [1, 2, 63, 1000, 1025, 4097, 65536]
# at Z = 5 none of those takes the one-copy regime (the any-Z kernel in the large LDS size): the
# smallest count that does
Z5_BIG = 373
PATTERNS = ["one", "mod", "random", "node"]
OUT_NAMES = ["count", "energy", "power_fx", "power", "dropped"]

# name: (node sizes, Z, shuffle_slots)
FLEETS = {
    "edges": ([0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 5000], 4, True),
    "z5": ([700, 300, 1300], 5, False),  # any-Z path, word by word
    "tiny": ([3], 4, False),
    "aligned": ([2048, 0, 2048, 0], 4, True),  # the batch ends on a tile, a node boundary and empty nodes on one
}
CASES = [("edges", k) for k in KINDS] + [(f, k) for f in ("z5", "tiny", "aligned") for k in ("proc", "pod")]


@pytest.fixture(scope="module", autouse=True)
def gpu_ready():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    accel.load()
    torch.cuda.set_stream(torch.cuda.Stream())  # every call below runs on a non-default stream


def test_the_group_counts_cross_every_regime():
    for zones, regimes in ((4, ["small", "small", "small", "big", "big", "pass", "pass"]),
                           (5, ["small", "small", "small", "pass", "pass", "pass", "pass"])):
        assert [group_regime(g, zones)[2] for g in N_GROUPS] == regimes
    assert group_regime(Z5_BIG - 1, 5)[2] == "small" and group_regime(Z5_BIG, 5) == (1, 1, "big")


def make(name, seed=7, **sim_args):
    sizes, zones, shuffle = FLEETS[name]
    L = fleet.make_layout(len(sizes), sizes, zones, seed=seed, shuffle_slots=shuffle, vm_frac=0.05)
    sim = fleet.FleetSim(L, seed=seed, **{"churn": 0.05, "read_error_frac": 0.1, **sim_args})
    return L, sim, accel.Accel(zones, **L.capacities())


def group_ids(pattern, row_off, n_groups, rng, none_frac=0.05):
    """u32 [n_rows]: the pattern's ids, about none_frac of them KACC_GROUP_NONE."""
    row_off = np.asarray(row_off, dtype=np.int64)
    n_rows = int(row_off[-1])
    if pattern == "one":
        g = np.full(n_rows, n_groups - 1, dtype=np.int64)
    elif pattern == "mod":
        g = np.arange(n_rows) % n_groups
    elif pattern == "random":
        g = rng.integers(0, n_groups, n_rows)
    else:  # constant per node: the rack case
        g = np.repeat((np.arange(len(row_off) - 1) * 7) % n_groups, np.diff(row_off))
    g = g.astype(np.uint32)
    g[rng.random(n_rows) < none_frac] = NONE
    return g


def dev_u32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


class Outputs:
    """Device outputs of one call for n_groups groups, prefilled with the sentinel."""

    def __init__(self, n_groups, Z):
        i32 = lambda m: torch.full((m,), SENT32, dtype=torch.int32, device="cuda")  # noqa: E731
        i64 = lambda m: torch.full((m,), SENT64, dtype=torch.int64, device="cuda")  # noqa: E731
        self.G, self.Z = n_groups, Z
        self.count, self.dropped = i32(n_groups), i32(n_groups)
        self.energy, self.power_fx, self.power = i64(n_groups * Z), i64(n_groups * Z), i64(n_groups * Z)

    def ptrs(self, only=None, skip=None):
        return [getattr(self, n).data_ptr() if (only is None or n == only) and n != skip else 0 for n in OUT_NAMES]

    def host(self):
        """count, energy, power_fx, power BITS, dropped — all unsigned."""
        u32 = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
        u64 = lambda t: t.cpu().numpy().view(np.uint64).reshape(self.G, self.Z)  # noqa: E731
        return u32(self.count), u64(self.energy), u64(self.power_fx), u64(self.power), u32(self.dropped)


def run_group(acc, kind, rows, group, n_groups, stream, mask=None, only=None, skip=None):
    o = Outputs(n_groups, acc.zones)
    o.group = dev_u32(group)
    o.mask = dev_u32(mask) if mask is not None else None
    acc.group_sums(KINDS[kind], rows, o.group.data_ptr(), n_groups, o.mask.data_ptr() if mask is not None else 0,
                   *o.ptrs(only, skip), stream)
    return o


def reference(state, kind, L, a, group, n_groups, mask=None, status=None):
    """The contract's outputs (power as bits) for the batch `a`; status overrides the batch's node_status."""
    st = a["node_status"] if status is None else status
    c, e, f, p, d = group_sums(state[f"{kind}_energy"], state[f"{kind}_power"], L.zones, a[f"{kind}_off"],
                               a[f"{kind}_slot"], st, mask, group, n_groups)
    return c, e, f, np.ascontiguousarray(p).view(np.uint64), d


def check(got, want, msg):
    for name, g, w in zip(OUT_NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{msg} {name}"
        np.testing.assert_array_equal(g, w, err_msg=f"{msg} {name}")


def expect_erange(acc, stream):
    with pytest.raises(accel.AccelError) as e:
        acc.sync(stream)
    assert e.value.code == accel.KACC_ERANGE
    assert "bits 0x2000" in str(e.value) and "8192=group sums" in str(e.value)
    assert "4096=select" in str(e.value)  # the earlier names of the message stay


def run_intervals(L, sim, acc, count, oracle=True):
    ora = Oracle(L.zones, **L.capacities()) if oracle else None
    s = current_stream_handle()
    for _ in range(count):
        a = sim.next_interval()
        t = to_device(a)
        acc.run_interval(interval_from_tensors(t, L.sizes()), s)
        if ora:
            ora.interval(a, L.sizes())
    acc.sync(s)
    return a, t, ora, s


@pytest.mark.parametrize("name,kind", CASES)
def test_sums_equal_the_contract_over_the_oracle(name, kind):
    L, sim, acc = make(name)
    ora = Oracle(L.zones, **L.capacities())
    s = current_stream_handle()
    rng = np.random.default_rng(17)
    contributed = 0
    for it in range(3):
        a = sim.next_interval()
        t = to_device(a)
        acc.run_interval(interval_from_tensors(t, L.sizes()), s)
        ora.interval(a, L.sizes())
        rows = top_rows_from_tensors(t, KINDS[kind])
        if name == "aligned" and kind == "proc":
            assert rows.n_rows == 4096  # two whole tiles
        for n_groups in N_GROUPS + ([Z5_BIG] if name == "z5" else []):
            for pattern in PATTERNS:
                group = group_ids(pattern, a[f"{kind}_off"], n_groups, rng)
                o = run_group(acc, kind, rows, group, n_groups, s)
                acc.sync(s)  # nothing raised
                want = reference(ora.state, kind, L, a, group, n_groups)
                check(o.host(), want, f"{name} {kind} it{it} G{n_groups} {pattern}")
                contributed = max(contributed, int(want[0].sum()))
    if a[f"{kind}_slot"].size > 3:  # the 3-process node has no pod
        assert contributed > 0
    acc.close()


def test_node_mask_and_shards_add_exactly():
    """Every third node listed and every third node dropped: the contract with those nodes' rows
    gone, and the two calls' u64 words add to the unmasked call's, word by word."""
    L, sim, acc = make("edges", seed=5)
    a, t, ora, s = run_intervals(L, sim, acc, 2)
    rng = np.random.default_rng(3)
    third = (np.arange(L.n_nodes) % 3 == 0).astype(np.uint32)
    for kind, n_groups in (("proc", 63), ("pod", 1025), ("proc", 4097)):
        rows = top_rows_from_tensors(t, KINDS[kind])
        group = group_ids("random", a[f"{kind}_off"], n_groups, rng)
        got = {}
        for label, mask in (("third", third), ("rest", 1 - third), ("none", np.zeros_like(third)),
                            ("high bit", third * 0x80000000), ("all", None)):
            o = run_group(acc, kind, rows, group, n_groups, s, mask=mask)
            acc.sync(s)
            got[label] = o.host()
            check(got[label], reference(ora.state, kind, L, a, group, n_groups, mask=mask), f"mask {label} {kind}")
        assert got["none"][0].sum() == 0 and got["all"][0].sum() > 0
        check(got["high bit"], got["third"], "any nonzero mask word lists")
        with np.errstate(over="ignore"):
            for i in (0, 1, 2, 4):
                np.testing.assert_array_equal(got["third"][i] + got["rest"][i], got["all"][i])
    acc.close()


def test_each_output_alone_and_each_output_left_out():
    """Every output alone (the others NULL) and every output NULL (the others given) hold the words
    of the full call; a NULL output's neighbours are untouched."""
    L, sim, acc = make("z5", seed=3)
    a, t, ora, s = run_intervals(L, sim, acc, 2)
    rows = top_rows_from_tensors(t, accel.KACC_KIND_PROC)
    rng = np.random.default_rng(1)
    for n_groups in (63, 4097):
        group = group_ids("random", a["proc_off"], n_groups, rng)
        want = reference(ora.state, "proc", L, a, group, n_groups)
        assert want[0].sum() > 0
        for i, name in enumerate(OUT_NAMES):
            for only, skip in ((name, None), (None, name)):
                o = run_group(acc, "proc", rows, group, n_groups, s, only=only, skip=skip)
                acc.sync(s)
                got = o.host()
                for j, other in enumerate(OUT_NAMES):
                    written = (other == only) if only else (other != skip)
                    if written:
                        np.testing.assert_array_equal(got[j], want[j], err_msg=f"{other} only={only} skip={skip}")
                    else:
                        assert np.all(got[j] == (SENT32 if j in (0, 4) else SENT64))
    acc.close()


def test_injected_values_are_dropped_and_counted():
    """Negative, NaN, ±Inf, 1e300 ratios in running process / container / VM slots, the same as
    stored pod powers plus a power exactly at ±2^50 µW and one just below: the contract over the
    tables downloaded afterwards; the dropped pairs are counted, and the sums are those of the
    tables with every dropped power replaced by zero."""
    L, sim, acc = make("edges", seed=11)
    a, t, _, s = run_intervals(L, sim, acc, 2, oracle=False)
    Z = L.zones
    special = np.array([np.nan, -1.5, -0.0, np.inf, 1e300, -np.inf, -1e-300, -3.25e7, 2.0 ** 50, -(2.0 ** 50),
                        np.nextafter(2.0 ** 50, 0.0), -np.nextafter(2.0 ** 50, 0.0)])
    rng = np.random.default_rng(3)
    for kind in ("proc", "ctr", "vm"):
        ratio = acc.download(f"{kind}_ratio")
        slots = (a[f"{kind}_slot"] & np.uint32(accel.KACC_SLOT_MASK)).astype(np.int64)
        pick = rng.choice(slots, size=min(400, slots.size), replace=False)
        ratio[pick] = special[rng.integers(0, 8, size=pick.size)]
        acc.upload(f"{kind}_ratio", ratio)
    pod = acc.download("pod_power").reshape(-1, Z)
    pslots = (a["pod_slot"] & np.uint32(accel.KACC_SLOT_MASK)).astype(np.int64)
    listed_pod = (a["node_status"][np.repeat(np.arange(L.n_nodes), np.diff(a["pod_off"].astype(np.int64)))]
                  & accel.KACC_NODE_READ_ERROR) == 0
    ppick = rng.choice(pslots[listed_pod], size=min(120, int(listed_pod.sum())), replace=False)
    pod[ppick, Z - 1] = special[np.arange(ppick.size) % special.size]  # every special value, the ±2^50 included
    acc.upload("pod_power", pod.reshape(-1))
    for kind in KINDS:
        state = {f"{kind}_energy": acc.download(f"{kind}_energy"), f"{kind}_power": acc.download(f"{kind}_power")}
        p = state[f"{kind}_power"]
        words, drop = fx(p)
        assert drop.any() and (p[~drop] < 0).any() and np.isnan(p).any() and np.isinf(p).any()
        if kind == "pod":
            assert (np.abs(p) == 2.0 ** 50).sum() >= 2 and drop[np.abs(p) == 2.0 ** 50].all()
            assert (np.abs(p) == np.nextafter(2.0 ** 50, 0.0)).any()
        zeroed = dict(state)
        zeroed[f"{kind}_power"] = np.where(drop, 0.0, p)
        rows = top_rows_from_tensors(t, KINDS[kind])
        for n_groups, pattern in ((2, "random"), (1000, "mod"), (4097, "random")):
            group = group_ids(pattern, a[f"{kind}_off"], n_groups, rng)
            o = run_group(acc, kind, rows, group, n_groups, s)
            acc.sync(s)
            got, want = o.host(), reference(state, kind, L, a, group, n_groups)
            check(got, want, f"injected {kind} G{n_groups}")
            assert got[4].sum() > 0  # some pair was dropped
            clean = reference(zeroed, kind, L, a, group, n_groups)
            assert clean[4].sum() == 0
            for i in (0, 1, 2, 3):  # the dropped rows still count and still add their energy
                np.testing.assert_array_equal(got[i], clean[i])
    acc.close()


def test_bad_group_id_and_bad_slot_are_left_out_and_reported():
    """One id equal to n_groups and one slot word past the capacity: KACC_ERANGE with the group
    bit at kacc_sync, no fault, every other row's contribution exact; the next correct call on the
    same context is right and raises nothing."""
    L, sim, acc = make("z5", seed=9, read_error_frac=0.0)
    a, t, ora, s = run_intervals(L, sim, acc, 1)
    rng = np.random.default_rng(2)
    n_rows = a["proc_slot"].size
    for n_groups in (63, 4097):
        good = group_ids("random", a["proc_off"], n_groups, rng, none_frac=0.0)
        rows = top_rows_from_tensors(t, accel.KACC_KIND_PROC)
        # the id alone
        group = good.copy()
        group[1234] = n_groups
        o = run_group(acc, "proc", rows, group, n_groups, s)
        expect_erange(acc, s)
        want = reference(ora.state, "proc", L, a, group, n_groups)
        assert want[0].sum() == n_rows - 1
        check(o.host(), want, "id == n_groups")
        # the slot alone, then both
        bad = dict(t)
        words = a["proc_slot"].copy()
        words[701] = 0xFFFFFFFF
        bad["proc_slot"] = dev_u32(words)
        bad_rows = top_rows_from_tensors(bad, accel.KACC_KIND_PROC)
        for g, left_out in ((good, 1), (group, 2)):
            o = run_group(acc, "proc", bad_rows, g, n_groups, s)
            expect_erange(acc, s)
            b = dict(a)
            b["proc_slot"] = words
            want = reference(ora.state, "proc", L, b, g, n_groups)
            assert want[0].sum() == n_rows - left_out
            check(o.host(), want, "slot past the capacity")
        o = run_group(acc, "proc", rows, good, n_groups, s)
        acc.sync(s)
        check(o.host(), reference(ora.state, "proc", L, a, good, n_groups), "after the clamp")
    acc.close()


def test_row_range_outside_the_batch_is_left_out():
    """n_rows short of the last node's range: that node's rows are left out (as a read-error
    node's would be), the others are right, and kacc_sync reports the group bit."""
    L, sim, acc = make("z5", seed=9, read_error_frac=0.0)
    a, t, ora, s = run_intervals(L, sim, acc, 1)
    rows = top_rows_from_tensors(t, accel.KACC_KIND_PROC)
    rows.n_rows = 1000  # nodes 0 and 1 own rows [0, 1000)
    group = group_ids("mod", a["proc_off"], 63, np.random.default_rng(4))
    o = run_group(acc, "proc", rows, group, 63, s)
    expect_erange(acc, s)
    want = reference(ora.state, "proc", L, a, group, 63,
                     status=np.array([0, 0, accel.KACC_NODE_READ_ERROR], dtype=np.uint32))
    assert 0 < want[0].sum() <= 1000
    check(o.host(), want, "short n_rows")
    acc.close()


def test_pods_by_namespace_equal_namespace_totals():
    """Pods grouped by their namespace: out_energy is kacc_namespace_totals' energy, bit for bit
    (no read errors: the CSR call sums every pod of the table)."""
    L = fleet.make_layout(32, 800, 4, seed=13, n_namespaces=7)
    sim = fleet.FleetSim(L, seed=13, churn=0.0)
    acc = accel.Accel(L.zones, **L.capacities())
    a, t, ora, s = run_intervals(L, sim, acc, 3)
    assert not (a["node_status"] & accel.KACC_NODE_READ_ERROR).any()
    np.testing.assert_array_equal(a["pod_slot"] & np.uint32(accel.KACC_SLOT_MASK), L.pod_slot)
    off, slots = L.namespace_csr()
    d = to_device({"o": off, "s": slots})
    n_ns = L.n_namespaces
    ns_e = torch.zeros(n_ns * L.zones, dtype=torch.int64, device="cuda")
    ns_p = torch.zeros(n_ns * L.zones, dtype=torch.float64, device="cuda")
    acc.namespace_totals(n_ns, d["o"].data_ptr(), d["s"].data_ptr(), ns_e.data_ptr(), ns_p.data_ptr(), s)
    rows = top_rows_from_tensors(t, accel.KACC_KIND_POD)
    o = run_group(acc, "pod", rows, L.pod_ns, n_ns, s)
    acc.sync(s)
    count, e, pfx, p, dropped = o.host()
    np.testing.assert_array_equal(e.reshape(-1), ns_e.cpu().numpy().view(np.uint64))
    np.testing.assert_array_equal(count, np.diff(off.astype(np.int64)).astype(np.uint32))
    assert e.any() and dropped.sum() == 0
    check(o.host(), reference(ora.state, "pod", L, a, L.pod_ns, n_ns), "pods by namespace")
    acc.close()


def test_lines_of_the_group_sums_byte_exact():
    """kacc_format_lines_dev on out_power with one label set per group: the bytes oracle/gofmt.py
    gives for the contract's values over the oracle's tables."""
    L, sim, acc = make("edges", seed=9)
    a, t, ora, s = run_intervals(L, sim, acc, 3)
    Z, G = L.zones, 63
    group = group_ids("random", a["proc_off"], G, np.random.default_rng(6))
    want = reference(ora.state, "proc", L, a, group, G)
    assert want[3].any()
    rows = top_rows_from_tensors(t, accel.KACC_KIND_PROC)
    o = run_group(acc, "proc", rows, group, G, s)
    labels = [label_pairs([("comm", f"worker-{g}"), ("state", "running")]).encode() for g in range(G)]
    label_off = np.r_[0, np.cumsum([len(x) for x in labels])].astype(np.uint64)
    d_labels = torch.from_numpy(np.frombuffer(b"".join(labels), dtype=np.uint8).copy()).cuda()
    d_loff = torch.from_numpy(label_off.view(np.int64)).cuda()
    zone_names = ["package", "core", "dram", "uncore"][:Z]
    metric = "kepler_process_cpu_watts"
    d_line_off = torch.zeros(G * Z + 1, dtype=torch.int64, device="cuda")
    args = (False, o.power.data_ptr(), G, metric, zone_names, d_labels.data_ptr(), d_loff.data_ptr(),
            d_line_off.data_ptr())
    total = acc.format_lines_dev(*args, stream=s)
    out = torch.zeros(total, dtype=torch.uint8, device="cuda")
    assert acc.format_lines_dev(*args, out_ptr=out.data_ptr(), out_cap=total, stream=s) == total
    acc.sync(s)
    vals = want[3].view(np.float64)
    text = b"".join(sample_line(metric, labels[g].decode(), zn, watts(float(vals[g, z]))).encode()
                    for g in range(G) for z, zn in enumerate(zone_names))
    assert bytes(out.cpu().numpy()) == text
    acc.close()


def test_two_calls_give_identical_bytes():
    """The same inputs twice, on this stream and on a second one: the same bytes in every output."""
    L, sim, acc = make("edges", seed=13)
    a, t, _, s = run_intervals(L, sim, acc, 3, oracle=False)
    rows = top_rows_from_tensors(t, accel.KACC_KIND_PROC)
    rng = np.random.default_rng(8)
    second = torch.cuda.Stream()
    for n_groups in (2, 1000, 65536):
        group = group_ids("random", a["proc_off"], n_groups, rng)
        first = run_group(acc, "proc", rows, group, n_groups, s)
        again = run_group(acc, "proc", rows, group, n_groups, s)
        acc.sync(s)
        with torch.cuda.stream(second):
            other = run_group(acc, "proc", rows, group, n_groups, second.cuda_stream)
            acc.sync(second.cuda_stream)
        assert first.host()[0].sum() > 0
        check(again.host(), first.host(), f"again G{n_groups}")
        check(other.host(), first.host(), f"second stream G{n_groups}")
    acc.close()


def test_host_errors_launch_nothing():
    L, sim, acc = make("tiny")
    a, t, _, s = run_intervals(L, sim, acc, 1, oracle=False)
    rows = top_rows_from_tensors(t, accel.KACC_KIND_PROC)
    o = Outputs(8, L.zones)
    group = dev_u32(np.zeros(3))
    lib, ctx = acc.lib, acc.ctx

    def call(kind=accel.KACC_KIND_PROC, r=rows, g=group.data_ptr(), n_groups=8, out=None, c=ctx):
        return lib.kacc_group_sums(c, kind, r, g, n_groups, None, *(o.ptrs() if out is None else out), s)

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
    assert call(g=None) == accel.KACC_EINVAL
    assert call(kind=4) == accel.KACC_EINVAL
    assert call(kind=-1) == accel.KACC_EINVAL
    assert call(n_groups=0) == accel.KACC_EINVAL
    assert call(n_groups=accel.KACC_GROUP_MAX + 1) == accel.KACC_EINVAL
    assert call(r=many) == accel.KACC_EINVAL
    assert call(out=[None] * 5) == accel.KACC_EINVAL
    acc.sync(s)  # nothing raised
    for got in o.host():  # and nothing written
        assert np.all(got == (SENT32 if got.dtype == np.uint32 else SENT64))
    # a batch without rows, and one without nodes, are no errors: every output is zero
    empty, none = accel.KaccTopRows(), accel.KaccTopRows()
    empty.n_nodes, empty.n_rows, empty.row_off, empty.slot, empty.node_status = 1, 0, group.data_ptr(), None, None
    none.n_nodes, none.n_rows, none.row_off, none.slot, none.node_status = 0, 0, rows.row_off, None, None
    for r in (empty, none):
        o = Outputs(8, L.zones)
        assert call(r=r, g=None) == accel.KACC_OK
        acc.sync(s)
        for got in o.host():
            assert not got.any()
    acc.close()
