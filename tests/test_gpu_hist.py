"""kacc_group_hist (value histograms of the running workloads by group) — MI355X only.

Whole outputs, bit for bit, against tests/hist_ref.py (the header's contract in numpy) fed from the
oracle's tables, after each of three intervals of the fleets of tests/test_gpu_group.py (churn and
read errors; node sizes that cross a 64-row word, a workgroup's step, several tiles, empty nodes, a
batch that ends on a tile) and of one fleet of its own around the kernels' 4096-row tile.  The (n_groups, n_bounds) shapes cross every LDS
capacity of the kernels (replicated counters, one copy, one pass more); the bounds are taken from
the oracle's own values, so bins are filled and rows sit exactly on a bound.  Every output is
prefilled with a pattern, so a word the call did not write shows.  No tolerance anywhere: every
output is an integer.
"""

import numpy as np
import pytest
import torch

from group_ref import contributing
from hist_ref import bound_keys, group_hist
from kepler_amd import accel, fleet
from kepler_amd.torch_batch import current_stream_handle, interval_from_tensors, to_device, top_rows_from_tensors
from oracle.oracle import Oracle
from plan_ref import MAX_COPIES, hist_regime as regime  # kacc_hist.hip's LDS plan, restated
from test_gpu_group import FLEETS, KINDS, dev_u32, group_ids, make, run_group, run_intervals
from top_ref import sort_key

pytestmark = pytest.mark.gpu

NONE = accel.KACC_GROUP_NONE
SENT64 = 0x5A5A5A5A5A5A5A5A  # output pre-fill
OUT_NAMES = ["bin", "cum", "sum", "nan", "unsummed"]
PATTERNS = ["one", "mod", "random", "node"]

# (n_groups, n_bounds); group is NULL for the first
SHAPES = [(1, 1), (1, 64), (2, 3), (63, 7), (1000, 15), (1025, 64), (16131, 64), (65536, 15),
          (204, 15), (205, 15),     # two copies | one copy of the counters
          (409, 15), (410, 15),     # the small | the large LDS size
          (1004, 15), (1005, 15),   # one copy | two passes
          (1920, 15), (1921, 15)]   # two | three passes
TABLES = [f"{k}_{q}" for k in KINDS for q in ("energy", "power")]
CASES = [("edges", t) for t in TABLES] + [(f, t) for f in ("z5", "tiny", "aligned") for t in ("proc_power", "pod_energy")]


def test_the_shapes_cross_every_capacity():
    assert regime(1, 1)[0] == MAX_COPIES and regime(63, 7)[0] > 1
    assert regime(204, 15) == (2, 1, "small") and regime(205, 15) == (1, 1, "small")
    assert regime(409, 15) == (1, 1, "small") and regime(410, 15) == (1, 1, "big")
    assert regime(1000, 15) == (1, 1, "big")
    assert regime(1004, 15) == (1, 1, "big") and regime(1005, 15) == (1, 2, "pass")
    assert regime(1920, 15) == (1, 2, "pass") and regime(1921, 15) == (1, 3, "pass")
    assert regime(1025, 64)[2] == "pass" and regime(16131, 64)[1] > 50 and regime(65536, 15)[1] > 50
    assert 65536 * 16 == accel.KACC_HIST_MAX_BINS and 16131 * 65 <= accel.KACC_HIST_MAX_BINS
    assert {regime(*s)[2] for s in SHAPES} == {"small", "big", "pass"}


@pytest.fixture(scope="module", autouse=True)
def gpu_ready():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    accel.load()
    torch.cuda.set_stream(torch.cuda.Stream())  # every call below runs on a non-default stream


def batch_values(table, zones, zone, a, state):
    kind = table.split("_")[0]
    slots = (a[f"{kind}_slot"] & np.uint32(accel.KACC_SLOT_MASK)).astype(np.int64)
    return np.ascontiguousarray(state[table].reshape(-1, zones)[slots, zone])


def make_bounds(vals, is_power, n_bounds):
    """n_bounds bounds (u64 bits, ascending by key) from the batch rows' own values: the value most
    rows share (rows equal to a bound), one above the maximum, 0.0 for a power, then quantiles of
    the present values; padded above the maximum when the rows hold fewer distinct values."""
    bits = vals.view(np.uint64)
    if is_power:
        bits = bits[~np.isnan(vals)]
    cand = []
    if bits.size:
        keys = sort_key(bits.view(np.float64) if is_power else bits, is_power)
        order = np.argsort(keys, kind="stable")
        uniq, counts = np.unique(bits, return_counts=True)
        cand.append(int(uniq[np.argmax(counts)]))
        top = bits[order[-1]]
        if is_power:
            cand.append(int(np.nextafter(top.view(np.float64), np.inf).view(np.uint64)))
            cand.append(0)  # +0.0
        elif int(top) < 2 ** 64 - 1:
            cand.append(int(top) + 1)
        q = np.linspace(0, bits.size - 1, 2 * n_bounds + 1).astype(np.int64)[1::2]
        cand += [int(b) for b in bits[order[q]]]
    pad = 1.0 if is_power else 1
    if cand:
        last = max(cand, key=lambda b: int(bound_keys([b], is_power)[0]))
        pad = max(float(np.uint64(last).view(np.float64)), 1.0) if is_power else last
    out, seen = [], set()
    for b in cand:
        k = int(bound_keys([b], is_power)[0])
        if k not in seen and len(out) < n_bounds and not (is_power and k == 0):
            seen.add(k)
            out.append(b)
    while len(out) < n_bounds:
        pad = pad * 2.0 if is_power else pad + 1
        b = int(np.float64(pad).view(np.uint64)) if is_power else int(pad)
        k = int(bound_keys([b], is_power)[0])
        if k not in seen:
            seen.add(k)
            out.append(b)
    out = np.array(out, dtype=np.uint64)
    return out[np.argsort(bound_keys(out, is_power), kind="stable")]


class Outputs:
    """Device outputs of one call, prefilled with the sentinel."""

    def __init__(self, n_groups, n_bounds):
        i64 = lambda m: torch.full((m,), SENT64, dtype=torch.int64, device="cuda")  # noqa: E731
        self.G, self.B1 = n_groups, n_bounds + 1
        self.bin, self.cum = i64(n_groups * self.B1), i64(n_groups * self.B1)
        self.sum, self.nan, self.unsummed = i64(n_groups), i64(n_groups), i64(n_groups)

    def ptrs(self, only=None):
        return [getattr(self, n).data_ptr() if only is None or n == only else 0 for n in OUT_NAMES]

    def host(self):
        u64 = lambda t: t.cpu().numpy().view(np.uint64)  # noqa: E731
        return (u64(self.bin).reshape(self.G, self.B1), u64(self.cum).reshape(self.G, self.B1), u64(self.sum),
                u64(self.nan), u64(self.unsummed))


def run_hist(acc, table, zone, rows, group, n_groups, bounds, stream, mask=None, only=None):
    o = Outputs(n_groups, len(bounds))
    # a batch without rows still passes an array: a NULL group means "one group" to the call
    o.group = dev_u32(group if group.size else np.zeros(1)) if group is not None else None
    o.mask = dev_u32(mask) if mask is not None else None
    acc.group_hist(table, zone, rows, o.group.data_ptr() if group is not None else 0, n_groups, bounds,
                   o.mask.data_ptr() if mask is not None else 0, *o.ptrs(only), stream)
    return o


def reference(state, table, L, zone, a, group, n_groups, bounds, mask=None, status=None):
    kind = table.split("_")[0]
    st = a["node_status"] if status is None else status
    return group_hist(state[table], table.endswith("power"), L.zones, zone, a[f"{kind}_off"], a[f"{kind}_slot"], st,
                      mask, group, n_groups, bounds)


def check(got, want, msg):
    for name, g, w in zip(OUT_NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{msg} {name}"
        np.testing.assert_array_equal(g, w, err_msg=f"{msg} {name}")


def expect_erange(acc, stream):
    with pytest.raises(accel.AccelError) as e:
        acc.sync(stream)
    assert e.value.code == accel.KACC_ERANGE
    assert "bits 0x4000" in str(e.value) and "16384=histogram" in str(e.value)
    assert "8192=group sums" in str(e.value)  # the earlier names of the message stay


@pytest.mark.parametrize("name,table", CASES)
def test_histograms_equal_the_contract_over_the_oracle(name, table):
    L, sim, acc = make(name)
    ora = Oracle(L.zones, **L.capacities())
    s = current_stream_handle()
    rng = np.random.default_rng(17)
    kind, is_power = table.split("_")[0], table.endswith("power")
    two_bins = on_a_bound = False
    for it in range(3):
        a = sim.next_interval()
        t = to_device(a)
        acc.run_interval(interval_from_tensors(t, L.sizes()), s)
        ora.interval(a, L.sizes())
        rows = top_rows_from_tensors(t, KINDS[kind])
        for zone in sorted({0, L.zones - 1}):
            vals = batch_values(table, L.zones, zone, a, ora.state)
            key = sort_key(vals, is_power)
            for i, (n_groups, n_bounds) in enumerate(SHAPES):
                bounds = make_bounds(vals, is_power, n_bounds)
                group = None if i == 0 else group_ids(PATTERNS[(i + it) % 4], a[f"{kind}_off"], n_groups, rng)
                o = run_hist(acc, table, zone, rows, group, n_groups, bounds, s)
                acc.sync(s)  # nothing raised
                want = reference(ora.state, table, L, zone, a, group, n_groups, bounds)
                check(o.host(), want, f"{name} {table} it{it} z{zone} G{n_groups} B{n_bounds}")
                # on the reference, so that the comparison is not vacuous
                ok = contributing(a[f"{kind}_off"], a[f"{kind}_slot"], a["node_status"], None,
                                  np.zeros(key.size, dtype=np.uint32) if group is None else group, n_groups)
                two_bins = two_bins or bool(((want[0] != 0).sum(axis=1) >= 2).any())
                on_a_bound = on_a_bound or bool(np.isin(key[ok], bound_keys(bounds, is_power)).any())
                assert (want[1][:, -1] == want[0].sum(axis=1)).all()
    if a[f"{kind}_slot"].size > 3:  # the 3-process node has no pod
        assert two_bins and on_a_bound
    acc.close()


def test_nodes_around_the_4096_row_tile():
    """kacc_hist.hip's tile is 4096 rows (512 lanes x 8): nodes that end one row before, on and one
    row after a tile, a one-row node, an empty one, and a batch that ends on a tile."""
    sizes = [4095, 1, 4096, 0, 4097, 4095]
    L = fleet.make_layout(len(sizes), sizes, 4, seed=7, shuffle_slots=True, vm_frac=0.05)
    sim = fleet.FleetSim(L, seed=7, churn=0.05, read_error_frac=0.1)
    acc = accel.Accel(L.zones, **L.capacities())
    a, t, ora, s = run_intervals(L, sim, acc, 2)
    assert a["proc_slot"].size == 4 * 4096
    rng = np.random.default_rng(4)
    rows = top_rows_from_tensors(t, accel.KACC_KIND_PROC)
    for table in ("proc_power", "proc_energy"):
        vals = batch_values(table, L.zones, 0, a, ora.state)
        for i, (n_groups, n_bounds) in enumerate(((1, 15), (63, 7), (1000, 15), (1921, 15))):
            bounds = make_bounds(vals, table.endswith("power"), n_bounds)
            group = None if i == 0 else group_ids(PATTERNS[i], a["proc_off"], n_groups, rng)
            o = run_hist(acc, table, 0, rows, group, n_groups, bounds, s)
            acc.sync(s)
            want = reference(ora.state, table, L, 0, a, group, n_groups, bounds)
            assert want[0].sum() > 4096
            check(o.host(), want, f"tile {table} G{n_groups}")
    acc.close()


def test_special_values_follow_the_rule():
    """NaN (both signs, payloads), -1.5, -0.0, ±Inf, 1e300, -1e-300 in running process / container /
    VM ratios and in stored pod powers; bounds -Inf, -1.5, -0.0, the smallest denormal, +Inf: the
    contract over the tables downloaded afterwards."""
    L, sim, acc = make("edges", seed=11)
    a, t, _, s = run_intervals(L, sim, acc, 2, oracle=False)
    Z = L.zones
    nans = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF],
                    dtype=np.uint64).view(np.float64)
    special = np.array([*nans, -1.5, -0.0, np.inf, 1e300, -np.inf, -1e-300])
    rng = np.random.default_rng(3)
    for kind in ("proc", "ctr", "vm"):
        ratio = acc.download(f"{kind}_ratio")
        slots = (a[f"{kind}_slot"] & np.uint32(accel.KACC_SLOT_MASK)).astype(np.int64)
        pick = rng.choice(slots, size=min(400, slots.size), replace=False)
        ratio[pick] = special[np.arange(pick.size) % special.size]
        acc.upload(f"{kind}_ratio", ratio)
    pod = acc.download("pod_power").reshape(-1, Z)
    pslots = (a["pod_slot"] & np.uint32(accel.KACC_SLOT_MASK)).astype(np.int64)
    listed_pod = (a["node_status"][np.repeat(np.arange(L.n_nodes), np.diff(a["pod_off"].astype(np.int64)))]
                  & accel.KACC_NODE_READ_ERROR) == 0
    ppick = rng.choice(pslots[listed_pod], size=min(120, int(listed_pod.sum())), replace=False)
    pod[ppick, Z - 1] = special[np.arange(ppick.size) % special.size]
    acc.upload("pod_power", pod.reshape(-1))
    bounds = np.array([-np.inf, -1.5, -0.0, 5e-324, np.inf]).view(np.uint64)
    for kind in KINDS:
        table = f"{kind}_power"
        state = {table: acc.download(table)}
        rows = top_rows_from_tensors(t, KINDS[kind])
        for (n_groups, pattern), zone in zip(((1, None), (2, "random"), (1000, "mod"), (1025, "random")),
                                             (Z - 1, Z - 1, 0 if kind != "pod" else Z - 1, Z - 1)):
            group = None if pattern is None else group_ids(pattern, a[f"{kind}_off"], n_groups, rng)
            o = run_hist(acc, table, zone, rows, group, n_groups, bounds, s)
            acc.sync(s)
            got, want = o.host(), reference(state, table, L, zone, a, group, n_groups, bounds)
            check(got, want, f"special {table} G{n_groups}")
            if kind == "pod" or n_groups != 1000:
                # NaN rows, unsummed rows, rows at -Inf, at -1.5, at the zeros and above +Inf's predecessor
                assert got[3].sum() > 0 and got[4].sum() > 0
                assert (got[0].sum(axis=0)[[0, 1, 2, 4]] > 0).all() and got[0][:, 5].sum() == 0
    acc.close()


def test_sums_and_counts_equal_the_group_sums():
    """The same call inputs through kacc_group_sums: out_sum is its power_fx (energy) column of the
    zone, out_cum's last column + out_nan its count."""
    L, sim, acc = make("edges", seed=5)
    a, t, ora, s = run_intervals(L, sim, acc, 2)
    rng = np.random.default_rng(5)
    third = (np.arange(L.n_nodes) % 3 != 0).astype(np.uint32)
    for table, n_groups, n_bounds, mask in (("proc_power", 63, 7, None), ("pod_power", 1000, 15, third),
                                            ("ctr_energy", 2, 3, None), ("vm_energy", 1025, 64, third),
                                            ("proc_energy", 4097, 15, None)):
        kind, is_power = table.split("_")[0], table.endswith("power")
        rows = top_rows_from_tensors(t, KINDS[kind])
        group = group_ids("random", a[f"{kind}_off"], n_groups, rng)
        for zone in (0, L.zones - 1):
            bounds = make_bounds(batch_values(table, L.zones, zone, a, ora.state), is_power, n_bounds)
            h = run_hist(acc, table, zone, rows, group, n_groups, bounds, s, mask=mask).host()
            count, e, pfx, _, _ = run_group(acc, kind, rows, group, n_groups, s, mask=mask).host()
            acc.sync(s)
            np.testing.assert_array_equal(h[2], (pfx if is_power else e)[:, zone])
            np.testing.assert_array_equal(h[1][:, -1] + h[3], count.astype(np.uint64))
            assert count.sum() > 0
    acc.close()


def test_node_mask_and_shards_add_exactly():
    """Every third node listed and its complement: the contract with those nodes' rows gone, and
    the two calls' words add to the unmasked call's, word by word."""
    L, sim, acc = make("edges", seed=5)
    a, t, ora, s = run_intervals(L, sim, acc, 2)
    rng = np.random.default_rng(3)
    third = (np.arange(L.n_nodes) % 3 == 0).astype(np.uint32)
    for table, n_groups, n_bounds in (("proc_power", 63, 7), ("pod_energy", 1025, 64), ("proc_energy", 1005, 15)):
        kind = table.split("_")[0]
        rows = top_rows_from_tensors(t, KINDS[kind])
        group = group_ids("random", a[f"{kind}_off"], n_groups, rng)
        bounds = make_bounds(batch_values(table, L.zones, 0, a, ora.state), table.endswith("power"), n_bounds)
        got = {}
        for label, mask in (("third", third), ("rest", 1 - third), ("none", np.zeros_like(third)),
                            ("high bit", third * 0x80000000), ("other", third * 7), ("all", None)):
            o = run_hist(acc, table, 0, rows, group, n_groups, bounds, s, mask=mask)
            acc.sync(s)
            got[label] = o.host()
            check(got[label], reference(ora.state, table, L, 0, a, group, n_groups, bounds, mask=mask),
                  f"mask {label} {table}")
        assert got["none"][0].sum() == 0 and not any(x.any() for x in got["none"]) and got["all"][0].sum() > 0
        check(got["high bit"], got["third"], "any nonzero mask word lists")
        check(got["other"], got["third"], "any nonzero mask word lists")
        with np.errstate(over="ignore"):
            for i in range(5):
                np.testing.assert_array_equal(got["third"][i] + got["rest"][i], got["all"][i])
    acc.close()


def test_each_output_alone():
    """Every output alone (the other four NULL) holds the words of the full call."""
    L, sim, acc = make("z5", seed=3)
    a, t, ora, s = run_intervals(L, sim, acc, 2)
    rows = top_rows_from_tensors(t, accel.KACC_KIND_PROC)
    rng = np.random.default_rng(1)
    for n_groups, n_bounds in ((63, 7), (1005, 15)):
        group = group_ids("random", a["proc_off"], n_groups, rng)
        bounds = make_bounds(batch_values("proc_power", L.zones, 4, a, ora.state), True, n_bounds)
        want = reference(ora.state, "proc_power", L, 4, a, group, n_groups, bounds)
        assert want[0].sum() > 0
        for i, name in enumerate(OUT_NAMES):
            o = run_hist(acc, "proc_power", 4, rows, group, n_groups, bounds, s, only=name)
            acc.sync(s)
            got = o.host()
            for j, other in enumerate(OUT_NAMES):
                if other == name:
                    np.testing.assert_array_equal(got[j], want[j], err_msg=f"{other} alone")
                else:
                    assert np.all(got[j] == SENT64)
    acc.close()


def test_bad_ids_slots_and_ranges_are_left_out_and_reported():
    """An id equal to n_groups, a slot word past the capacity, a node whose row range leaves the
    batch: each is left out, every other word stays exact and kacc_sync raises KACC_ERANGE with
    the histogram bit; KACC_GROUP_NONE raises nothing."""
    L, sim, acc = make("z5", seed=9, read_error_frac=0.0)
    a, t, ora, s = run_intervals(L, sim, acc, 1)
    rng = np.random.default_rng(2)
    n_rows = a["proc_slot"].size
    vals = batch_values("proc_energy", L.zones, 0, a, ora.state)
    for n_groups, n_bounds in ((63, 7), (1005, 15)):
        bounds = make_bounds(vals, False, n_bounds)
        good = group_ids("random", a["proc_off"], n_groups, rng, none_frac=0.0)
        rows = top_rows_from_tensors(t, accel.KACC_KIND_PROC)
        ref = lambda b, g, **kw: reference(ora.state, "proc_energy", L, 0, b, g, n_groups, bounds, **kw)  # noqa: E731
        # the id alone
        group = good.copy()
        group[1234] = n_groups
        o = run_hist(acc, "proc_energy", 0, rows, group, n_groups, bounds, s)
        expect_erange(acc, s)
        want = ref(a, group)
        assert want[1][:, -1].sum() == n_rows - 1
        check(o.host(), want, "id == n_groups")
        # KACC_GROUP_NONE in its place: silent
        group[1234] = NONE
        o = run_hist(acc, "proc_energy", 0, rows, group, n_groups, bounds, s)
        acc.sync(s)
        check(o.host(), want, "KACC_GROUP_NONE")
        # the slot
        bad = dict(t)
        words = a["proc_slot"].copy()
        words[701] = 0xFFFFFFFF
        bad["proc_slot"] = dev_u32(words)
        bad_rows = top_rows_from_tensors(bad, accel.KACC_KIND_PROC)
        o = run_hist(acc, "proc_energy", 0, bad_rows, good, n_groups, bounds, s)
        expect_erange(acc, s)
        b = dict(a)
        b["proc_slot"] = words
        want = ref(b, good)
        assert want[1][:, -1].sum() == n_rows - 1
        check(o.host(), want, "slot past the capacity")
        # the row range: n_rows short of the last node's range (nodes 0 and 1 own rows [0, 1000))
        short = top_rows_from_tensors(t, accel.KACC_KIND_PROC)
        short.n_rows = 1000
        o = run_hist(acc, "proc_energy", 0, short, good, n_groups, bounds, s)
        expect_erange(acc, s)
        want = ref(a, good, status=np.array([0, 0, accel.KACC_NODE_READ_ERROR], dtype=np.uint32))
        assert 0 < want[1][:, -1].sum() <= 1000
        check(o.host(), want, "short n_rows")
        # and the next correct call is right and raises nothing
        o = run_hist(acc, "proc_energy", 0, rows, good, n_groups, bounds, s)
        acc.sync(s)
        check(o.host(), ref(a, good), "after the clamp")
    acc.close()


def test_two_calls_and_a_second_stream_give_identical_bytes():
    L, sim, acc = make("edges", seed=13)
    a, t, _, s = run_intervals(L, sim, acc, 3, oracle=False)
    rows = top_rows_from_tensors(t, accel.KACC_KIND_PROC)
    rng = np.random.default_rng(8)
    second = torch.cuda.Stream()
    state = {"proc_power": acc.download("proc_power")}
    for n_groups, n_bounds in ((2, 3), (1000, 15), (65536, 15)):
        bounds = make_bounds(batch_values("proc_power", L.zones, 0, a, state), True, n_bounds)
        group = group_ids("random", a["proc_off"], n_groups, rng)
        first = run_hist(acc, "proc_power", 0, rows, group, n_groups, bounds, s)
        again = run_hist(acc, "proc_power", 0, rows, group, n_groups, bounds, s)
        acc.sync(s)
        with torch.cuda.stream(second):
            other = run_hist(acc, "proc_power", 0, rows, group, n_groups, bounds, second.cuda_stream)
            acc.sync(second.cuda_stream)
        assert first.host()[0].sum() > 0
        check(again.host(), first.host(), f"again G{n_groups}")
        check(other.host(), first.host(), f"second stream G{n_groups}")
    acc.close()


def test_host_errors_launch_nothing():
    L, sim, acc = make("tiny")
    a, t, _, s = run_intervals(L, sim, acc, 1, oracle=False)
    rows = top_rows_from_tensors(t, accel.KACC_KIND_PROC)
    o = Outputs(8, 2)
    group = dev_u32(np.zeros(3))
    lib, ctx = acc.lib, acc.ctx
    f64 = lambda *v: np.array(v, dtype=np.float64).view(np.uint64)  # noqa: E731
    T = accel.TABLE_INDEX

    def call(table=T["proc_power"], zone=0, r=rows, g=group.data_ptr(), n_groups=8, bounds=f64(1.0, 2.0),
             n_bounds=None, out=None, c=ctx):
        b = None if bounds is None else np.ascontiguousarray(bounds, dtype=np.uint64)
        n = (0 if b is None else b.size) if n_bounds is None else n_bounds
        return lib.kacc_group_hist(c, table, zone, r, g, n_groups, None if b is None else b.ctypes.data, n, None,
                                   *(o.ptrs() if out is None else out), s)

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
    assert call(bounds=None, n_bounds=2) == E
    assert call(g=None) == E  # NULL group with n_groups 8
    assert call(table=T["node_power"]) == E
    assert call(table=T["proc_ratio"]) == E
    assert call(table=-1) == E
    assert call(zone=L.zones) == E
    assert call(n_bounds=0) == E
    assert call(table=T["proc_energy"], bounds=np.arange(65, dtype=np.uint64)) == E
    assert call(n_groups=0) == E
    assert call(n_groups=accel.KACC_GROUP_MAX + 1) == E
    assert call(n_groups=61681, bounds=f64(*range(1, 17))) == E  # 61681 * 17 = KACC_HIST_MAX_BINS + 1
    for bad in (f64(2.0, 1.0), f64(0.0, -0.0), f64(1.0, 1.0), f64(np.nan), f64(1.0, np.nan)):
        assert call(bounds=bad) == E
    assert call(table=T["proc_energy"], bounds=np.array([5, 5], dtype=np.uint64)) == E
    assert call(r=many) == E
    assert call(out=[None] * 5) == E
    acc.sync(s)  # nothing raised
    for got in o.host():  # and nothing written
        assert np.all(got == SENT64)
    # the bits of a NaN are a valid energy bound
    assert call(table=T["proc_energy"], bounds=f64(1.0, np.nan)) == accel.KACC_OK
    acc.sync(s)
    # a batch without rows, and one without nodes, are no errors: every output is zero
    empty, none = accel.KaccTopRows(), accel.KaccTopRows()
    empty.n_nodes, empty.n_rows, empty.row_off, empty.slot, empty.node_status = 1, 0, group.data_ptr(), None, None
    none.n_nodes, none.n_rows, none.row_off, none.slot, none.node_status = 0, 0, rows.row_off, None, None
    for r in (empty, none):
        for g, n_groups in ((None, 1), (group.data_ptr(), 8)):
            o = Outputs(n_groups, 2)
            assert call(r=r, g=g, n_groups=n_groups) == accel.KACC_OK
            acc.sync(s)
            for got in o.host():
                assert not got.any()
    acc.close()
