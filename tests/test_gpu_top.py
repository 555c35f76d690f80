"""kacc_top_nodes / kacc_top_fleet (top consumers of the running workloads) — MI355X only.

Whole output arrays against tests/top_ref.py (the header's order rule in numpy) fed from the
oracle's tables, after each of three intervals of fleets with churn and read errors: the first
interval has every power 0 (a pure tie-break by row), later ones ~30 % rows at 0 (ties inside
the lists).  Node sizes cross every boundary of the selection kernel (wave, first sort trigger,
the 2048-entry buffer, several buffers), k runs from 1 to KACC_TOP_MAX, past a node's and past
the fleet's rows.  Special values (NaN, -0.0, negatives, Inf), consistency with the scrape and
kacc_unpack, the clamp of a bad slot word, host errors and a second stream have their own cases.
"""

import numpy as np
import pytest
import torch

from kepler_amd import accel, fleet
from kepler_amd.torch_batch import current_stream_handle, interval_from_tensors, to_device, top_rows_from_tensors
from oracle.oracle import Oracle
from top_ref import top_lists

pytestmark = pytest.mark.gpu

KS = [1, 10, 64, 1000, 1024]
KINDS = {"proc": accel.KACC_KIND_PROC, "ctr": accel.KACC_KIND_CTR, "vm": accel.KACC_KIND_VM,
         "pod": accel.KACC_KIND_POD}
ALL_TABLES = [f"{kind}_{what}" for kind in KINDS for what in ("energy", "power")]

# name: (node sizes, Z, shuffle_slots)
FLEETS = {
    "edges": ([0, 1, 63, 64, 65, 2047, 2048, 2049, 5000], 4, True),
    "many": ([300, 7, 0, 1000, 64] * 14, 2, False),
    "tiny": ([3], 4, False),
    "z5": ([700, 300, 1300], 5, False),
}
CASES = [("edges", t) for t in ALL_TABLES] + [(f, t) for f in ("many", "tiny", "z5")
                                              for t in ("proc_energy", "proc_power", "pod_energy", "pod_power")]


@pytest.fixture(scope="module", autouse=True)
def gpu_ready():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    accel.load()
    torch.cuda.set_stream(torch.cuda.Stream())


def make(name, seed=7):
    sizes, zones, shuffle = FLEETS[name]
    L = fleet.make_layout(len(sizes), sizes, zones, seed=seed, shuffle_slots=shuffle, vm_frac=0.05)
    sim = fleet.FleetSim(L, seed=seed, churn=0.05, read_error_frac=0.1)
    return L, sim, accel.Accel(zones, **L.capacities())


class Outputs:
    """Device output arrays of one call, prefilled with a pattern neither a result nor the fill."""

    def __init__(self, lists, k, fleet_call):
        n = lists * k
        i32 = lambda m: torch.full((max(m, 1),), -2, dtype=torch.int32, device="cuda")  # noqa: E731
        self.lists, self.k, self.fleet_call = lists, k, fleet_call
        self.count, self.row, self.slot, self.node = i32(lists), i32(n), i32(n), i32(n)
        self.value = torch.full((max(n, 1),), -2, dtype=torch.int64, device="cuda")

    def host(self):
        u32 = lambda t, m: t.cpu().numpy().view(np.uint32)[:m]  # noqa: E731
        n = self.lists * self.k
        shape = (self.k,) if self.fleet_call else (self.lists, self.k)
        out = [u32(self.count, self.lists), u32(self.row, n).reshape(shape), u32(self.slot, n).reshape(shape)]
        if self.fleet_call:
            out.append(u32(self.node, n))
        out.append(self.value.cpu().numpy().view(np.uint64)[:n].reshape(shape))
        return tuple(out)


def run_top(acc, table, zone, k, rows, n_nodes, stream, fleet_call):
    o = Outputs(1 if fleet_call else n_nodes, k, fleet_call)
    if fleet_call:
        acc.top_fleet(table, zone, k, rows, o.count.data_ptr(), o.row.data_ptr(), o.slot.data_ptr(),
                      o.node.data_ptr(), o.value.data_ptr(), stream)
    else:
        acc.top_nodes(table, zone, k, rows, o.count.data_ptr(), o.row.data_ptr(), o.slot.data_ptr(),
                      o.value.data_ptr(), stream)
    return o


def check(got, want, msg):
    """Whole output arrays, bit for bit (the values are u64: a NaN must keep its bits)."""
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.dtype.kind == "u"
        np.testing.assert_array_equal(g, w, err_msg=f"{msg} output {i}")


def check_both(acc, tables, L, a, t, table, zone, k, stream, msg):
    kind = table.split("_")[0]
    is_power = table.endswith("power")
    want = top_lists(tables[table], L.zones, zone, is_power, a[f"{kind}_off"], a[f"{kind}_slot"], a["node_status"], k)
    rows = top_rows_from_tensors(t, KINDS[kind])
    on = run_top(acc, table, zone, k, rows, L.n_nodes, stream, False)
    of = run_top(acc, table, zone, k, rows, L.n_nodes, stream, True)
    acc.sync(stream)
    check(on.host(), want["nodes"], f"{msg} top_nodes")
    check(of.host(), want["fleet"], f"{msg} top_fleet")
    return want


@pytest.mark.parametrize("name,table", CASES)
def test_lists_equal_the_order_rule_over_the_oracle(name, table):
    L, sim, acc = make(name)
    ora = Oracle(L.zones, **L.capacities())
    s = current_stream_handle()
    listed = 0
    for it in range(3):
        a = sim.next_interval()
        t = to_device(a)
        acc.run_interval(interval_from_tensors(t, L.sizes()), s)
        ora.interval(a, L.sizes())
        for zone in sorted({0, L.zones - 1}):
            for k in KS:
                want = check_both(acc, ora.state, L, a, t, table, zone, k, s, f"{name} {table} it{it} z{zone} k{k}")
                listed += int(want["fleet"][0][0])
    assert listed > 0 or a[f"{table.split('_')[0]}_slot"].size == 0  # the 3-process node has no pod
    acc.close()


def test_special_values_follow_the_order_rule():
    """NaN, negative, -0.0, +Inf and huge ratios in running process slots, and the same as stored
    pod powers: the expectation is the order rule over the downloaded power table."""
    L, sim, acc = make("edges", seed=11)
    s = current_stream_handle()
    for _ in range(2):
        a = sim.next_interval()
        t = to_device(a)
        acc.run_interval(interval_from_tensors(t, L.sizes()), s)
    acc.sync(s)
    # two NaNs with a payload, one of them with the sign bit: a NaN keeps its bits in out_value
    NAN_NEG, NAN_POS = 0xFFF8000000000123, 0x7FF8000000BEEF01
    special = np.concatenate([np.array([np.nan, -1.5, -0.0, np.inf, 1e300, -np.inf, -1e-300]).view(np.uint64),
                              np.array([NAN_NEG, NAN_POS], dtype=np.uint64)]).view(np.float64)
    rng = np.random.default_rng(3)
    ratio = acc.download("proc_ratio")
    slots = (a["proc_slot"] & np.uint32(accel.KACC_SLOT_MASK)).astype(np.int64)
    pick = rng.choice(slots, size=min(400, slots.size), replace=False)
    ratio[pick] = special[rng.integers(0, special.size, size=pick.size)]
    # rows of the 63-, 64- and 65-row nodes, which k = 1024 lists whole
    ratio[slots[[5, 70, 130]]] = special[[7, 8, 7]]
    acc.upload("proc_ratio", ratio)
    Z = L.zones
    pod = acc.download("pod_power").reshape(-1, Z)
    pslots = (a["pod_slot"] & np.uint32(accel.KACC_SLOT_MASK)).astype(np.int64)
    ppick = rng.choice(pslots, size=min(60, pslots.size), replace=False)
    pod[ppick, Z - 1] = special[rng.integers(0, special.size, size=ppick.size)]
    pod[pslots[[0, pslots.size // 2, pslots.size - 1]], Z - 1] = special[[7, 8, 7]]
    acc.upload("pod_power", pod.reshape(-1))
    assert NAN_NEG in acc.download("pod_power").view(np.uint64).tolist()  # a stored word keeps its bits
    for table in ("proc_power", "pod_power"):
        tables = {table: acc.download(table)}
        v = tables[table].reshape(-1, Z)[:, Z - 1]
        assert np.isnan(v).any() and (v < 0).any() and np.isinf(v).any() and np.signbit(v[v == 0]).any()
        for k in (10, 1024):
            want = check_both(acc, tables, L, a, t, table, Z - 1, k, s, f"special {table} k{k}")
        # the order rule, stated on the list itself: +Inf first; NaN only after every number
        fv = want["fleet"][4][: int(want["fleet"][0][0])].view(np.float64)
        assert fv[0] == np.inf
        nan_at = np.flatnonzero(np.isnan(fv))
        assert nan_at.size == 0 or nan_at[0] + nan_at.size == fv.size
    # every pod of a listed node is in the k = 1024 fleet list: the payload NaNs with their bits
    # (check_both compared the device's lists with these, bit for bit)
    listed_bits = want["fleet"][4].tolist()
    assert NAN_NEG in listed_bits or NAN_POS in listed_bits
    acc.close()


@pytest.mark.parametrize("table", ["proc_power", "pod_power", "ctr_energy"])
def test_values_are_the_scrape_and_unpack(table):
    """out_value is the slot's element of kacc_table_download bit for bit, and kacc_unpack on
    out_slot returns rows whose `zone` column is out_value."""
    L, sim, acc = make("many", seed=5)
    s = current_stream_handle()
    for _ in range(2):
        a = sim.next_interval()
        t = to_device(a)
        acc.run_interval(interval_from_tensors(t, L.sizes()), s)
    kind = table.split("_")[0]
    Z, zone, k = L.zones, L.zones - 1, 64
    rows = top_rows_from_tensors(t, KINDS[kind])
    for fleet_call in (False, True):
        o = run_top(acc, table, zone, k, rows, L.n_nodes, s, fleet_call)
        n = o.lists * k
        ue = torch.zeros((n * Z,), dtype=torch.int64, device="cuda")
        up = torch.zeros((n * Z,), dtype=torch.float64, device="cuda")
        acc.sync(s)
        out = o.host()
        count, slot, value = out[0], out[2].reshape(o.lists, k), out[-1].reshape(o.lists, k)
        live = np.arange(k)[None, :] < count[:, None]
        assert live.any()
        scrape = acc.download(table).view(np.uint64).reshape(-1, Z)
        np.testing.assert_array_equal(value[live], scrape[slot[live].astype(np.int64), zone])
        # unpack the listed slots (entries past a count: slot 0, not compared)
        words = torch.from_numpy(np.where(live, slot, 0).astype(np.uint32).view(np.int32).reshape(-1)).cuda()
        acc.unpack(KINDS[kind], n, words.data_ptr(), 0, ue.data_ptr(), up.data_ptr(), s)
        acc.sync(s)
        src = up.cpu().numpy().view(np.uint64) if table.endswith("power") else ue.cpu().numpy().view(np.uint64)
        np.testing.assert_array_equal(src.reshape(o.lists, k, Z)[:, :, zone][live], value[live])
    acc.close()


def test_bad_slot_word_is_clamped_and_reported():
    """A slot word past the capacity is left out and raises KACC_ERANGE with the top-list bit;
    the next correct call on the same context gives the right lists."""
    L, sim, acc = make("z5", seed=9)
    ora = Oracle(L.zones, **L.capacities())
    s = current_stream_handle()
    a = sim.next_interval()
    t = to_device(a)
    acc.run_interval(interval_from_tensors(t, L.sizes()), s)
    ora.interval(a, L.sizes())
    acc.sync(s)
    bad = dict(t)
    words = a["proc_slot"].copy()
    words[701] = 0xFFFFFFFF
    bad["proc_slot"] = torch.from_numpy(words.view(np.int32)).cuda()
    rows = top_rows_from_tensors(bad, accel.KACC_KIND_PROC)
    for fleet_call in (False, True):
        o = run_top(acc, "proc_energy", 0, 1024, rows, L.n_nodes, s, fleet_call)
        with pytest.raises(accel.AccelError) as e:
            acc.sync(s)
        assert e.value.code == accel.KACC_ERANGE
        assert "bits 0x200" in str(e.value) and "512=top list" in str(e.value)
        out = o.host()
        assert out[0].tolist() == ([1024] if fleet_call else [700, 299, 1024])  # row 701 is left out
        assert 701 not in out[1].reshape(-1).tolist()
    check_both(acc, ora.state, L, a, t, "proc_energy", 0, 1024, s, "after the clamp")
    acc.close()


def test_row_range_outside_the_batch_is_left_out():
    """n_rows short of the last node's range: that node lists nothing (as a read-error node
    would), the others are right, and kacc_sync reports the top-list bit."""
    L, sim, acc = make("z5", seed=9)
    s = current_stream_handle()
    a = sim.next_interval()
    t = to_device(a)
    acc.run_interval(interval_from_tensors(t, L.sizes()), s)
    acc.sync(s)
    rows = top_rows_from_tensors(t, accel.KACC_KIND_PROC)
    rows.n_rows = 1000  # nodes 0 and 1 own rows [0, 1000)
    want = top_lists(acc.download("proc_energy"), L.zones, 1, False, a["proc_off"], a["proc_slot"],
                     np.array([0, 0, accel.KACC_NODE_READ_ERROR], dtype=np.uint32), 64)
    for fleet_call in (False, True):
        o = run_top(acc, "proc_energy", 1, 64, rows, L.n_nodes, s, fleet_call)
        with pytest.raises(accel.AccelError) as e:
            acc.sync(s)
        assert e.value.code == accel.KACC_ERANGE and "bits 0x200" in str(e.value)
        check(o.host(), want["fleet" if fleet_call else "nodes"], "short n_rows")
    acc.close()


def test_host_errors_launch_nothing():
    L, sim, acc = make("tiny")
    s = current_stream_handle()
    a = sim.next_interval()
    t = to_device(a)
    acc.run_interval(interval_from_tensors(t, L.sizes()), s)
    rows = top_rows_from_tensors(t, accel.KACC_KIND_PROC)
    for fleet_call in (False, True):
        for table, zone, k in (("proc_power", 0, 0), ("proc_power", 0, accel.KACC_TOP_MAX + 1),
                               ("proc_power", L.zones, 10), ("node_power", 0, 10), ("proc_ratio", 0, 10)):
            with pytest.raises(accel.AccelError) as e:
                run_top(acc, table, zone, k, rows, L.n_nodes, s, fleet_call)
            assert e.value.code == accel.KACC_EINVAL
    acc.sync(s)  # nothing ran, nothing raised
    acc.close()


def test_second_stream_gives_the_same_lists():
    """top_fleet on a second stream that waits for the interval's event, the next interval after
    it: the lists of the one-stream run."""
    results = []
    for two in (False, True):
        L, sim, acc = make("many", seed=13)
        main = torch.cuda.current_stream()
        side = torch.cuda.Stream() if two else main
        got = []
        for _ in range(3):
            a = sim.next_interval()
            t = to_device(a)
            o = Outputs(1, 100, True)  # filled on the main stream, before the side stream waits for it
            acc.run_interval(interval_from_tensors(t, L.sizes()), main.cuda_stream)
            side.wait_stream(main)
            rows = top_rows_from_tensors(t, accel.KACC_KIND_PROC)
            acc.top_fleet("proc_power", 0, 100, rows, o.count.data_ptr(), o.row.data_ptr(), o.slot.data_ptr(),
                          o.node.data_ptr(), o.value.data_ptr(), side.cuda_stream)
            main.wait_stream(side)  # the next interval rewrites what the lists read
            got.append((o, t))
        acc.sync(side.cuda_stream)
        acc.sync(main.cuda_stream)
        results.append([o.host() for o, _ in got])
        acc.close()
    for one, other in zip(*results):
        for x, y in zip(one, other):
            np.testing.assert_array_equal(x, y)
    assert int(results[0][-1][0][0]) == 100
