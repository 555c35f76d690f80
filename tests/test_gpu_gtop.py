"""kacc_group_top (top-K running workloads per caller-defined group) — MI355X only.

Whole outputs, byte for byte, against tests/gtop_ref.py (the header's contract in numpy) fed from the
oracle's tables, after each of three intervals of the fleets of tests/test_gpu_group.py (churn and
read errors; node sizes that cross a 64-row word, a workgroup's step, several tiles, empty nodes, a
batch that ends on a tile).  The (n_groups, k) shapes cross both counter regimes of the kernels
(LDS counters, replicated or one copy; global atomics) and both sort granularities (a wave, a
workgroup); uploaded tables make the tie cut, each key digit and each row digit decide alone.  Every
output is prefilled with a pattern, so a word the call did not write shows.  No tolerance anywhere.
"""

import numpy as np
import pytest
import torch

from gtop_ref import group_top, merge_shards
from kepler_amd import accel, fleet
from kepler_amd.torch_batch import current_stream_handle, interval_from_tensors, to_device, top_rows_from_tensors
from oracle.oracle import Oracle
from plan_ref import gtop_regime as regime  # kacc_gtop.hip's counter plan, restated
from test_gpu_group import KINDS, dev_u32, group_ids, make, run_group, run_intervals
from test_gpu_quant import run_quant
from test_gpu_top import run_top
from top_ref import sort_key

pytestmark = pytest.mark.gpu

NONE = accel.KACC_GROUP_NONE
FILL = 0xFFFFFFFF
SENT32, SENT64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A  # output pre-fill: neither a result nor the fill
OUT_NAMES = ["count", "row", "slot", "node", "value"]

# kacc_gtop.hip's, restated: a wave sorts a segment of at most 64 entries, a workgroup one of at
# most KACC_TOP_MAX
WAVE_K = 64


def sorter(k):
    return "wave" if k <= WAVE_K else "workgroup"


# (n_groups, k); group is NULL for n_groups 1 in the contract test
SHAPES = [(1, 1), (1, 1024), (7, 10), (63, 64), (64, 65), (65, 2), (1000, 3), (1024, 1024), (65536, 1), (65536, 16)]
TABLES = [f"{k}_{q}" for k in KINDS for q in ("energy", "power")]
CASES = [("edges", t) for t in TABLES] + [(f, t) for f in ("z5", "tiny", "aligned") for t in ("proc_power", "pod_energy")]
PATTERNS = ["one", "mod", "random", "node"]
# the contract test's shape per pattern: both regimes, both sorters
PATTERN_SHAPE = {"one": (1, 100), "mod": (63, 64), "random": (7, 10), "node": (1000, 3)}


def test_the_shapes_cross_every_regime_and_both_sorters():
    assert regime(1) == (32, "lds") and regime(7)[0] == 8 and regime(31) == (2, "lds") and regime(32) == (1, "lds")
    assert regime(63) == (1, "lds") and regime(64) == (1, "lds") and regime(65) == (0, "global")
    assert regime(1000) == regime(1024) == regime(65536) == (0, "global")
    assert {regime(g) for g, _ in SHAPES} == {(32, "lds"), (8, "lds"), (1, "lds"), (0, "global")}
    assert sorter(64) == "wave" and sorter(65) == "workgroup"
    assert {(regime(g)[1], sorter(k)) for g, k in SHAPES} == {(w, s) for w in ("lds", "global") for s in ("wave", "workgroup")}
    for g, k in SHAPES:
        assert g * k <= accel.KACC_GROUP_TOP_MAX_ITEMS and k <= accel.KACC_TOP_MAX
    assert (1024, 1024) in SHAPES and (65536, 16) in SHAPES  # the item limit, both ways
    assert {(regime(g)[1], sorter(k)) for g, k in PATTERN_SHAPE.values()} == {("lds", "wave"), ("lds", "workgroup"),
                                                                             ("global", "wave")}


@pytest.fixture(scope="module", autouse=True)
def gpu_ready():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    accel.load()
    torch.cuda.set_stream(torch.cuda.Stream())  # every call below runs on a non-default stream


class Outputs:
    """Device outputs of one call, prefilled with the sentinel."""

    def __init__(self, n_groups, k):
        i32 = lambda m: torch.full((m,), SENT32, dtype=torch.int32, device="cuda")  # noqa: E731
        self.G, self.k = n_groups, k
        self.count, self.row, self.slot, self.node = i32(n_groups), i32(n_groups * k), i32(n_groups * k), i32(n_groups * k)
        self.value = torch.full((n_groups * k,), SENT64, dtype=torch.int64, device="cuda")

    def ptrs(self, only=None, skip=None):
        return [getattr(self, n).data_ptr() if (only is None or n == only) and n != skip else 0 for n in OUT_NAMES]

    def host(self):
        """count u32 [G]; row, slot, node u32 [G, k]; value u64 [G, k]."""
        u32 = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
        return (u32(self.count), *(u32(getattr(self, n)).reshape(self.G, self.k) for n in OUT_NAMES[1:4]),
                self.value.cpu().numpy().view(np.uint64).reshape(self.G, self.k))


def run_gtop(acc, table, zone, k, rows, group, n_groups, stream, mask=None, only=None, skip=None):
    o = Outputs(n_groups, k)
    # a batch without rows still passes an array: a NULL group means "one group" to the call
    o.group = dev_u32(group if group.size else np.zeros(1)) if group is not None else None
    o.mask = dev_u32(mask) if mask is not None else None
    acc.group_top(table, zone, k, rows, o.group.data_ptr() if group is not None else 0, n_groups,
                  o.mask.data_ptr() if mask is not None else 0, *o.ptrs(only, skip), stream)
    return o


def reference(state, table, L, zone, a, group, n_groups, k, mask=None, status=None):
    kind = table.split("_")[0]
    st = a["node_status"] if status is None else status
    return group_top(state[table], table.endswith("power"), L.zones, zone, a[f"{kind}_off"], a[f"{kind}_slot"], st, mask,
                     group, n_groups, k)


def check(got, want, msg):
    for name, g, w in zip(OUT_NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{msg} {name}"
        np.testing.assert_array_equal(g, w, err_msg=f"{msg} {name}")


def expect_erange(acc, stream):
    with pytest.raises(accel.AccelError) as e:
        acc.sync(stream)
    assert e.value.code == accel.KACC_ERANGE
    assert "bits 0x200" in str(e.value) and "512=top list" in str(e.value)


@pytest.mark.parametrize("name,table", CASES)
def test_lists_equal_the_contract_over_the_oracle(name, table):
    L, sim, acc = make(name)
    ora = Oracle(L.zones, **L.capacities())
    s = current_stream_handle()
    rng = np.random.default_rng(17)
    kind = table.split("_")[0]
    listed = cut = 0
    for it in range(3):
        a = sim.next_interval()
        t = to_device(a)
        acc.run_interval(interval_from_tensors(t, L.sizes()), s)
        ora.interval(a, L.sizes())
        rows = top_rows_from_tensors(t, KINDS[kind])
        for zone in sorted({0, L.zones - 1}):
            for pattern, (n_groups, k) in PATTERN_SHAPE.items():
                group = None if pattern == "one" else group_ids(pattern, a[f"{kind}_off"], n_groups, rng)
                o = run_gtop(acc, table, zone, k, rows, group, n_groups, s)
                acc.sync(s)  # nothing raised
                want = reference(ora.state, table, L, zone, a, group, n_groups, k)
                check(o.host(), want, f"{name} {table} it{it} z{zone} {pattern}")
                # on the reference, so that the comparison is not vacuous
                listed += int(want[0].sum())
                cut += int((want[0] == k).sum())
    if a[f"{kind}_slot"].size > 3:  # the 3-process node has no pod
        assert listed > 0 and cut > 0
    acc.close()


def test_shapes_across_every_regime_and_both_sorters():
    L, sim, acc = make("edges", seed=5)
    a, t, ora, s = run_intervals(L, sim, acc, 2)
    rng = np.random.default_rng(4)
    for table in ("proc_power", "pod_energy"):
        kind = table.split("_")[0]
        rows = top_rows_from_tensors(t, KINDS[kind])
        for i, (n_groups, k) in enumerate(SHAPES):
            for pattern in (PATTERNS[i % 4], PATTERNS[(i + 2) % 4]):
                if pattern == "one" and n_groups == 1:
                    group = None
                else:
                    group = group_ids(pattern, a[f"{kind}_off"], n_groups, rng)
                o = run_gtop(acc, table, 0, k, rows, group, n_groups, s)
                acc.sync(s)
                want = reference(ora.state, table, L, 0, a, group, n_groups, k)
                assert want[0].sum() > 0
                check(o.host(), want, f"shape {table} G{n_groups} k{k} {pattern}")
    acc.close()


def test_identities_with_the_top_lists_the_sums_and_the_quantiles():
    """The header's four identities, on the device's own outputs, byte for byte."""
    L, sim, acc = make("edges", seed=5)
    a, t, ora, s = run_intervals(L, sim, acc, 2)
    rng = np.random.default_rng(12)
    for table in ("proc_power", "pod_energy", "pod_power", "ctr_energy"):
        kind = table.split("_")[0]
        rows = top_rows_from_tensors(t, KINDS[kind])
        off = np.asarray(a[f"{kind}_off"], dtype=np.int64)
        for k in (1, 100, 1024):  # kacc_top_fleet: all five outputs
            o = run_gtop(acc, table, 0, k, rows, None, 1, s)
            f = run_top(acc, table, 0, k, rows, L.n_nodes, s, True)
            acc.sync(s)
            got, want = o.host(), f.host()
            assert want[0][0] > 0
            for g, w in zip(got, want):
                np.testing.assert_array_equal(g.reshape(-1), w.reshape(-1), err_msg=f"fleet {table} k{k}")
        node_ids = np.repeat(np.arange(L.n_nodes), np.diff(off)).astype(np.uint32)
        for k in (10, 100):  # kacc_top_nodes: count, row, slot, value
            o = run_gtop(acc, table, 0, k, rows, node_ids, L.n_nodes, s)
            n = run_top(acc, table, 0, k, rows, L.n_nodes, s, False)
            acc.sync(s)
            count, row, slot, node, value = o.host()
            check((count, row, slot, value), n.host(), f"nodes {table} k{k}")
            assert ((node == np.arange(L.n_nodes, dtype=np.uint32)[:, None]) | (node == FILL)).all()
        # kacc_group_sums' count
        n_groups, k = 40, 5
        group = group_ids("random", off, n_groups, rng)
        o = run_gtop(acc, table, 0, k, rows, group, n_groups, s)
        sums = run_group(acc, kind, rows, group, n_groups, s)
        acc.sync(s)
        count, _, _, _, value = o.host()
        np.testing.assert_array_equal(count, np.minimum(sums.host()[0], k))
        assert (count == k).any()
        if table.endswith("energy"):  # kacc_group_quantiles' maximum
            q = run_quant(acc, table, 0, rows, group, n_groups, [1.0], s)
            acc.sync(s)
            lo = q.host()[2][:, 0]
            some = count > 0
            assert some.any()
            np.testing.assert_array_equal(value[some, 0], lo[some])
    acc.close()


def upload_zone(acc, table, zones, zone, slots, words):
    """Writes the u64 `words` into (slots, zone) of `table`; returns the table as the device holds it."""
    is_power = table.endswith("power")
    tab = acc.download(table).view(np.uint64).reshape(-1, zones)
    tab[slots, zone] = words
    acc.upload(table, tab.reshape(-1).view(np.float64 if is_power else np.uint64))
    return {table: acc.download(table)}


@pytest.mark.parametrize("table", ["pod_energy", "proc_energy"])
def test_ties_decide_alone(table):
    L, sim, acc = make("edges", seed=11, read_error_frac=0.0)
    a, t, _, s = run_intervals(L, sim, acc, 1, oracle=False)
    kind, Z = table.split("_")[0], L.zones
    off = a[f"{kind}_off"]
    slots = (a[f"{kind}_slot"] & np.uint32(accel.KACC_SLOT_MASK)).astype(np.int64)
    rows = top_rows_from_tensors(t, KINDS[kind])
    rng = np.random.default_rng(21)
    # every listed value equal: a list is its group's k lowest rows
    state = upload_zone(acc, table, Z, 1, slots, np.full(slots.size, 777, dtype=np.uint64))
    for n_groups, k in ((1, 100), (7, 10), (7, 1024), (100, 3)):
        group = None if n_groups == 1 else group_ids("mod", off, n_groups, rng, none_frac=0.0)
        o = run_gtop(acc, table, 1, k, rows, group, n_groups, s)
        acc.sync(s)
        got = o.host()
        check(got, reference(state, table, L, 1, a, group, n_groups, k), f"equal {table} G{n_groups} k{k}")
        for g in range(n_groups):
            mine = np.arange(slots.size) if group is None else np.flatnonzero(group == g)
            np.testing.assert_array_equal(got[1][g, :got[0][g]], mine[:k])
    # two values: the cut inside the block of the lower value, on its edge, or inside the upper one
    n_groups, k = 6, 30
    group = group_ids("mod", off, n_groups, rng, none_frac=0.0)
    words = np.full(slots.size, 5, dtype=np.uint64)
    for g, high in enumerate((0, 10, 29, 30, 31, 200)):  # group g has `high` rows of the upper value
        mine = np.flatnonzero(group == g)
        assert mine.size > 2 * k or table == "pod_energy"
        words[rng.permutation(mine)[:high]] = 9
    state = upload_zone(acc, table, Z, 1, slots, words)
    o = run_gtop(acc, table, 1, k, rows, group, n_groups, s)
    acc.sync(s)
    want = reference(state, table, L, 1, a, group, n_groups, k)
    check(o.host(), want, f"two values {table}")
    if table == "proc_energy":
        assert [(want[4][g] == 9).sum() for g in range(n_groups)] == [0, 10, 29, 30, 30, 30]
    acc.close()


def test_the_third_row_digit_decides():
    """36 nodes x 2048 processes, all energies equal: the tie cut alone selects, by three row digits.
    With every node listed a group's 1024 lowest rows end near row 7,167; behind a mask the lists
    start at row 67,584, or at row 63,488 and end past row 65,536."""
    sizes = [2048] * 36
    L = fleet.make_layout(len(sizes), sizes, 4, seed=7, vm_frac=0.05)
    sim = fleet.FleetSim(L, seed=7, churn=0.0, read_error_frac=0.0)
    acc = accel.Accel(4, **L.capacities())
    a, t, _, s = run_intervals(L, sim, acc, 1, oracle=False)
    n_rows = a["proc_slot"].size
    assert n_rows == 73728 > 65536
    slots = (a["proc_slot"] & np.uint32(accel.KACC_SLOT_MASK)).astype(np.int64)
    state = upload_zone(acc, "proc_energy", 4, 0, slots, np.full(n_rows, 123456, dtype=np.uint64))
    rows = top_rows_from_tensors(t, accel.KACC_KIND_PROC)
    rng = np.random.default_rng(2)
    for n_groups, k, first_node in ((7, 1024, 0), (7, 1024, 33), (7, 1024, 31), (2, 1024, 33), (7, 100, 33)):
        group = group_ids("mod", a["proc_off"], n_groups, rng, none_frac=0.0)
        mask = (np.arange(36) >= first_node).astype(np.uint32) if first_node else None
        o = run_gtop(acc, "proc_energy", 0, k, rows, group, n_groups, s, mask=mask)
        acc.sync(s)
        got = o.host()
        check(got, reference(state, "proc_energy", L, 0, a, group, n_groups, k, mask=mask), f"G{n_groups} k{k} from {first_node}")
        listed = got[1][got[1] != FILL]
        assert listed.min() == first_node * 2048
        if first_node == 31:
            assert listed.min() < 65536 < listed.max() and (got[0] == k).all()
        if first_node == 33 and n_groups == 7 and k == 1024:
            assert (got[0] < k).all()  # 6,144 rows in 7 groups: nothing is cut
    acc.close()


@pytest.mark.parametrize("table", ["pod_energy", "proc_energy"])
def test_each_key_digit_decides_alone(table):
    """Group b holds energies that differ in byte b alone: only that digit pass can order them."""
    L, sim, acc = make("edges", seed=11, read_error_frac=0.0)
    a, t, _, s = run_intervals(L, sim, acc, 1, oracle=False)
    kind, Z = table.split("_")[0], L.zones
    slots = (a[f"{kind}_slot"] & np.uint32(accel.KACC_SLOT_MASK)).astype(np.int64)
    per = 40
    assert np.unique(slots).size == slots.size >= 8 * per
    rng = np.random.default_rng(6)
    pick = rng.permutation(slots.size)[:8 * per].reshape(8, per)  # the crafted rows, anywhere in the batch
    group = np.full(slots.size, NONE, dtype=np.uint32)
    words = np.zeros(slots.size, dtype=np.uint64)
    base = np.uint64(0x4142434445464748)
    for b in range(8):
        group[pick[b]] = b
        digits = rng.permutation(256)[:per].astype(np.uint64)
        clear = ~(np.uint64(0xFF) << np.uint64(8 * b))
        words[pick[b]] = (base & clear) | (digits << np.uint64(8 * b))
    state = upload_zone(acc, table, Z, Z - 1, slots, words)
    rows = top_rows_from_tensors(t, KINDS[kind])
    for n_groups in (8, 9, 70):  # LDS counters, global counters; the last groups stay empty
        for k in (1, 7, 39, 40, 64, 65):
            o = run_gtop(acc, table, Z - 1, k, rows, group, n_groups, s)
            acc.sync(s)
            got = o.host()
            check(got, reference(state, table, L, Z - 1, a, group, n_groups, k), f"digit {table} G{n_groups} k{k}")
            for b in range(8):
                best = np.sort(words[pick[b]])[::-1][:k]
                np.testing.assert_array_equal(got[4][b, :best.size], best)
            assert (got[0][:8] == min(k, per)).all() and not got[0][8:].any()
    acc.close()


def test_special_powers_keep_their_rank_and_their_bits():
    L, sim, acc = make("edges", seed=11, read_error_frac=0.0)
    a, t, _, s = run_intervals(L, sim, acc, 1, oracle=False)
    Z = L.zones
    slots = (a["pod_slot"] & np.uint32(accel.KACC_SLOT_MASK)).astype(np.int64)
    NAN_NEG, NAN_POS = 0xFFF8000000000123, 0x7FF8000000BEEF01
    f64 = lambda *v: np.array(v, dtype=np.float64).view(np.uint64)  # noqa: E731
    special = np.concatenate([f64(np.inf, -np.inf, -0.0, 0.0, -1.5, -1e-300, 1e300, 2.5, 2.5),
                              np.array([NAN_NEG, NAN_POS, NAN_NEG], dtype=np.uint64)])
    rng = np.random.default_rng(5)
    n_groups = 3
    group = np.full(slots.size, NONE, dtype=np.uint32)
    words = np.zeros(slots.size, dtype=np.uint64)
    pick = rng.permutation(slots.size)[:n_groups * special.size].reshape(n_groups, special.size)
    for g in range(n_groups):
        group[pick[g]] = g
        words[pick[g]] = special[rng.permutation(special.size)]
    state = upload_zone(acc, "pod_power", Z, 0, slots, words)
    assert NAN_NEG in state["pod_power"].view(np.uint64).tolist()  # a stored word keeps its bits
    rows = top_rows_from_tensors(t, accel.KACC_KIND_POD)
    for n_groups_call in (n_groups, 80):
        for k in (special.size, 5, 10, 64, 100):
            o = run_gtop(acc, "pod_power", 0, k, rows, group, n_groups_call, s)
            acc.sync(s)
            got = o.host()
            check(got, reference(state, "pod_power", L, 0, a, group, n_groups_call, k), f"special G{n_groups_call} k{k}")
        count, row, _, _, value = got  # k = 100: every row of a group
        for g in range(n_groups):
            assert count[g] == special.size
            v, r = value[g, :special.size], row[g, :special.size]
            p = v.view(np.float64)
            assert p[0] == np.inf and p[1] == 1e300 and p[2] == p[3] == 2.5 and r[2] < r[3]
            assert p[4] == 0 and p[5] == 0 and r[4] < r[5]  # the zeros share a key: row order
            assert sorted(v[4:6].tolist()) == [0, 1 << 63]  # and keep their own bits
            assert p[6] == -1e-300 and p[7] == -1.5 and p[8] == -np.inf
            assert np.isnan(p[9:]).all() and (np.diff(r[9:].astype(np.int64)) > 0).all()  # NaN last, by row
            assert sorted(v[9:].tolist()) == sorted([NAN_NEG, NAN_POS, NAN_NEG])
    acc.close()


def test_two_calls_a_second_stream_and_another_row_order():
    L, sim, acc = make("edges", seed=13)
    a, t, _, s = run_intervals(L, sim, acc, 3, oracle=False)
    rows = top_rows_from_tensors(t, accel.KACC_KIND_PROC)
    rng = np.random.default_rng(8)
    second = torch.cuda.Stream()
    # a second batch: the same slots, every node's rows listed in reverse
    off = np.asarray(a["proc_off"], dtype=np.int64)
    flip = np.concatenate([np.arange(off[n + 1] - 1, off[n] - 1, -1) for n in range(L.n_nodes)]).astype(np.int64)
    turned = dict(t)
    turned["proc_slot"] = dev_u32(a["proc_slot"][flip])
    turned_rows = top_rows_from_tensors(turned, accel.KACC_KIND_PROC)
    for table in ("proc_power", "proc_energy"):
        state = {table: acc.download(table)}
        compared = 0
        for n_groups, k in ((1, 1024), (7, 10), (1000, 3), (65536, 16)):
            group = None if n_groups == 1 else group_ids("random", a["proc_off"], n_groups, rng)
            first = run_gtop(acc, table, 0, k, rows, group, n_groups, s)
            again = run_gtop(acc, table, 0, k, rows, group, n_groups, s)
            other_order = run_gtop(acc, table, 0, k, turned_rows, None if group is None else group[flip], n_groups, s)
            acc.sync(s)
            with torch.cuda.stream(second):
                other = run_gtop(acc, table, 0, k, rows, group, n_groups, second.cuda_stream)
                acc.sync(second.cuda_stream)
            one, two = first.host(), other_order.host()
            assert one[0].sum() > 0
            check(again.host(), one, f"again {table} G{n_groups}")
            check(other.host(), one, f"second stream {table} G{n_groups}")
            # another row order is another batch: the contract on it, and against the first order
            # the same counts and, wherever a list's values are distinct, the same value sequence;
            # a list that holds its whole group (no tie with a row left out) has the same slots too
            b = dict(a)
            b["proc_slot"] = a["proc_slot"][flip]
            check(two, reference(state, table, L, 0, b, None if group is None else group[flip], n_groups, k),
                  f"reversed rows {table} G{n_groups}")
            np.testing.assert_array_equal(two[0], one[0])
            # the row behind a full list, where the limits leave room for it: is its key another one?
            longer = None
            if k < accel.KACC_TOP_MAX and n_groups * (k + 1) <= accel.KACC_GROUP_TOP_MAX_ITEMS:
                longer = reference(state, table, L, 0, a, group, n_groups, k + 1)
            is_power = table.endswith("power")
            for g in range(min(n_groups, 2000)):  # list by list: the first groups are enough
                c = int(one[0][g])
                v = one[4][g, :c]
                if np.unique(v).size != c:
                    continue
                np.testing.assert_array_equal(two[4][g, :c], v)
                compared += c > 1
                whole = c < k
                if not whole and longer is not None:
                    tail = longer[4][g, k - 1:k + 1]
                    key = sort_key(tail.view(np.float64) if is_power else tail, is_power)
                    whole = longer[0][g] == k or key[0] != key[1]
                if whole:  # no tie with a row left out: the same rows, so the same slots
                    np.testing.assert_array_equal(two[2][g, :c], one[2][g, :c])
                    np.testing.assert_array_equal(flip[two[1][g, :c]], one[1][g, :c])
        assert compared > 0
    acc.close()


def test_node_masks_and_shards_merge_exactly():
    L, sim, acc = make("edges", seed=5)
    a, t, ora, s = run_intervals(L, sim, acc, 2)
    rng = np.random.default_rng(3)
    third = (np.arange(L.n_nodes) % 3 == 0).astype(np.uint32)
    for table, n_groups, k in (("proc_power", 63, 20), ("pod_energy", 7, 100), ("proc_energy", 1, 1024), ("pod_power", 70, 3)):
        kind = table.split("_")[0]
        rows = top_rows_from_tensors(t, KINDS[kind])
        group = None if n_groups == 1 else group_ids("random", a[f"{kind}_off"], n_groups, rng)
        got = {}
        for label, mask in (("third", third), ("rest", 1 - third), ("none", np.zeros_like(third)),
                            ("high bit", third * 0x80000000), ("all", None)):
            o = run_gtop(acc, table, 0, k, rows, group, n_groups, s, mask=mask)
            acc.sync(s)
            got[label] = o.host()
            check(got[label], reference(ora.state, table, L, 0, a, group, n_groups, k, mask=mask), f"mask {label} {table}")
        assert got["none"][0].sum() == 0 and (got["none"][1] == FILL).all() and not got["none"][4].any()
        check(got["high bit"], got["third"], "any nonzero mask word lists")
        assert got["all"][0].sum() > 0
        check(merge_shards([got["third"], got["rest"]], table.endswith("power"), k), got["all"], f"shards {table}")
        # the largest node flagged with a read error
        status = np.asarray(a["node_status"], dtype=np.uint32).copy()
        status[L.n_nodes - 1] |= accel.KACC_NODE_READ_ERROR
        flagged = dict(t)
        flagged["node_status"] = dev_u32(status)
        o = run_gtop(acc, table, 0, k, top_rows_from_tensors(flagged, KINDS[kind]), group, n_groups, s)
        acc.sync(s)
        check(o.host(), reference(ora.state, table, L, 0, a, group, n_groups, k, status=status), f"read error {table}")
    acc.close()


def test_each_output_alone_and_each_output_left_out():
    """Every output alone (the others NULL) and every output NULL (the others given) hold the words
    of the full call; a NULL output's neighbours are untouched."""
    L, sim, acc = make("z5", seed=3)
    a, t, ora, s = run_intervals(L, sim, acc, 2)
    rows = top_rows_from_tensors(t, accel.KACC_KIND_PROC)
    rng = np.random.default_rng(1)
    for n_groups, k in ((7, 10), (70, 65)):
        group = group_ids("random", a["proc_off"], n_groups, rng)
        want = reference(ora.state, "proc_power", L, 4, a, group, n_groups, k)
        assert want[0].sum() > 0
        for name in OUT_NAMES:
            for kw in ({"only": name}, {"skip": name}):
                o = run_gtop(acc, "proc_power", 4, k, rows, group, n_groups, s, **kw)
                acc.sync(s)
                for other, g, w in zip(OUT_NAMES, o.host(), want):
                    if (other == name) == ("only" in kw):
                        np.testing.assert_array_equal(g, w, err_msg=f"{other} with {kw}")
                    else:
                        assert np.all(g == (SENT64 if other == "value" else SENT32))
    acc.close()


def test_bad_ids_slots_and_ranges_are_left_out_and_reported():
    """An id equal to n_groups, a slot word past the capacity, a node whose row range leaves the
    batch: each is left out, every other word stays exact and kacc_sync raises KACC_ERANGE with
    the top lists' bit; KACC_GROUP_NONE raises nothing."""
    L, sim, acc = make("z5", seed=9, read_error_frac=0.0)
    a, t, ora, s = run_intervals(L, sim, acc, 1)
    rng = np.random.default_rng(2)
    n_rows = a["proc_slot"].size
    k = 400  # the lists hold every row
    for n_groups in (7, 70):
        good = group_ids("random", a["proc_off"], n_groups, rng, none_frac=0.0)
        rows = top_rows_from_tensors(t, accel.KACC_KIND_PROC)
        ref = lambda b, g, **kw: reference(ora.state, "proc_energy", L, 0, b, g, n_groups, k, **kw)  # noqa: E731
        # the id alone
        group = good.copy()
        group[1234] = n_groups
        o = run_gtop(acc, "proc_energy", 0, k, rows, group, n_groups, s)
        expect_erange(acc, s)
        want = ref(a, group)
        assert want[0].sum() == n_rows - 1 or n_groups == 7
        assert 1234 not in want[1]
        check(o.host(), want, "id == n_groups")
        # KACC_GROUP_NONE in its place: silent
        group[1234] = NONE
        o = run_gtop(acc, "proc_energy", 0, k, rows, group, n_groups, s)
        acc.sync(s)
        check(o.host(), want, "KACC_GROUP_NONE")
        # the slot
        bad = dict(t)
        words = a["proc_slot"].copy()
        words[701] = 0xFFFFFFFF
        bad["proc_slot"] = dev_u32(words)
        o = run_gtop(acc, "proc_energy", 0, k, top_rows_from_tensors(bad, accel.KACC_KIND_PROC), good, n_groups, s)
        expect_erange(acc, s)
        b = dict(a)
        b["proc_slot"] = words
        want = ref(b, good)
        assert 701 not in want[1]
        check(o.host(), want, "slot past the capacity")
        # the row range: n_rows short of the last node's range (nodes 0 and 1 own rows [0, 1000))
        short = top_rows_from_tensors(t, accel.KACC_KIND_PROC)
        short.n_rows = 1000
        o = run_gtop(acc, "proc_energy", 0, k, short, good, n_groups, s)
        expect_erange(acc, s)
        want = ref(a, good, status=np.array([0, 0, accel.KACC_NODE_READ_ERROR], dtype=np.uint32))
        assert 0 < want[0].sum() <= 1000
        check(o.host(), want, "short n_rows")
        # and the next correct call is right and raises nothing
        o = run_gtop(acc, "proc_energy", 0, k, rows, good, n_groups, s)
        acc.sync(s)
        check(o.host(), ref(a, good), "after the clamp")
    acc.close()


def test_small_cases_and_host_errors_launch_nothing():
    L, sim, acc = make("tiny", read_error_frac=0.0)
    a, t, _, s = run_intervals(L, sim, acc, 1, oracle=False)
    rows = top_rows_from_tensors(t, accel.KACC_KIND_PROC)
    o = Outputs(8, 10)
    group = dev_u32(np.zeros(3))
    lib, ctx = acc.lib, acc.ctx
    T = accel.TABLE_INDEX

    def call(table=T["proc_power"], zone=0, k=10, r=rows, g=group.data_ptr(), n_groups=8, out=None, c=ctx):
        return lib.kacc_group_top(c, table, zone, k, r, g, n_groups, None, *(o.ptrs() if out is None else out), s)

    no_off, no_slot, many = (accel.KaccTopRows() for _ in range(3))
    for r in (no_off, no_slot, many):
        r.n_nodes, r.n_rows, r.row_off, r.slot, r.node_status = (rows.n_nodes, rows.n_rows, rows.row_off, rows.slot,
                                                                 rows.node_status)
    no_off.row_off = None
    no_slot.slot = None
    many.n_nodes = L.n_nodes + 1
    E = accel.KACC_EINVAL
    assert call(c=None) == E
    assert call(r=None) == E
    assert call(r=no_off) == E
    assert call(r=no_slot) == E
    assert call(g=None) == E  # NULL group with n_groups 8
    assert call(table=T["node_power"]) == E
    assert call(table=T["proc_ratio"]) == E
    assert call(table=-1) == E
    assert call(zone=L.zones) == E
    assert call(k=0) == E
    assert call(k=1025) == E
    assert call(n_groups=0) == E
    assert call(n_groups=accel.KACC_GROUP_MAX + 1) == E
    assert call(n_groups=1025, k=1024) == E  # 1024 x 1024 = KACC_GROUP_TOP_MAX_ITEMS
    assert call(n_groups=65536, k=17) == E
    assert call(r=many) == E
    assert call(out=[None] * 5) == E
    acc.sync(s)  # nothing raised
    for name, got in zip(OUT_NAMES, o.host()):  # and nothing written
        assert np.all(got == (SENT64 if name == "value" else SENT32))
    # 1024 groups x k = 1024 passes the size check: three rows in group 0
    big = Outputs(1024, 1024)
    assert call(n_groups=1024, k=1024, out=big.ptrs()) == accel.KACC_OK
    acc.sync(s)
    count, row, slot, node, value = big.host()
    assert count[0] == 3 and not count[1:].any() and sorted(row[0, :3].tolist()) == [0, 1, 2]
    assert (row.reshape(-1)[3:] == FILL).all() and (node.reshape(-1)[3:] == FILL).all() and not value.reshape(-1)[3:].any()
    # two identical calls: identical bytes
    again = Outputs(1024, 1024)
    assert call(n_groups=1024, k=1024, out=again.ptrs()) == accel.KACC_OK
    acc.sync(s)
    check(again.host(), (count, row, slot, node, value), "again")
    # a batch without rows, and one without nodes, are no errors: counts 0 and all fill
    empty, none = accel.KaccTopRows(), accel.KaccTopRows()
    empty.n_nodes, empty.n_rows, empty.row_off, empty.slot, empty.node_status = 1, 0, group.data_ptr(), None, None
    none.n_nodes, none.n_rows, none.row_off, none.slot, none.node_status = 0, 0, rows.row_off, None, None
    for r in (empty, none):
        for g, n_groups, k in ((None, 1, 10), (group.data_ptr(), 8, 10), (group.data_ptr(), 8, 100)):
            e = Outputs(n_groups, k)
            assert call(r=r, g=g, n_groups=n_groups, k=k, out=e.ptrs()) == accel.KACC_OK
            acc.sync(s)
            count, row, slot, node, value = e.host()
            assert not count.any() and not value.any()
            assert (row == FILL).all() and (slot == FILL).all() and (node == FILL).all()
    acc.close()
