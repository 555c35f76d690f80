"""kacc_group_quantiles (exact quantiles of the running workloads by group) — MI355X only.

Whole outputs, bit for bit, against tests/quant_ref.py (the header's contract in numpy) fed from the
oracle's tables, after each of three intervals of the fleets of tests/test_gpu_group.py (churn and
read errors; node sizes that cross a 64-row word, a workgroup's step, several tiles, empty nodes, a
batch that ends on a tile).  The (n_groups, n_phi) shapes cross every counter regime of the kernels
(replicated LDS counters, one copy, global atomics); crafted tables make each digit pass and the
successor step decide alone.  Every output is prefilled with a pattern, so a word the call did not
write shows.  No tolerance anywhere: weight and value are compared as bits.
"""

import numpy as np
import pytest
import torch

from group_ref import contributing
from hist_ref import bound_keys
from kepler_amd import accel
from kepler_amd.torch_batch import current_stream_handle, interval_from_tensors, to_device, top_rows_from_tensors
from oracle.oracle import Oracle
from plan_ref import quant_regime as regime  # kacc_quant.hip's counter plan, restated
from quant_ref import EMPTY_NAN, group_quantiles
from test_gpu_group import KINDS, dev_u32, group_ids, make, run_group, run_intervals
from test_gpu_hist import run_hist

pytestmark = pytest.mark.gpu

NONE = accel.KACC_GROUP_NONE
SENT64 = 0x5A5A5A5A5A5A5A5A  # output pre-fill
OUT_NAMES = ["count", "nan", "lo", "hi", "weight", "value"]
PHI5 = [0.0, 0.5, 0.9, 0.99, 1.0]
PHI1 = [1.0 / 3.0]
PHI8 = [0.5, 0.0, 1.0, 0.99, 0.9, 1.0 / 3.0, 0.25, 0.75]

# (n_groups, n_phi); group is NULL for n_groups 1
SHAPES = [(1, 1), (1, 8), (65536, 1), (8192, 8), (7, 1), (3, 5),
          (31, 1), (32, 1), (4, 8),     # two copies | one copy of the counters
          (64, 1), (8, 8), (65, 1), (13, 5),  # one copy | global atomics
          (1000, 3)]
TABLES = [f"{k}_{q}" for k in KINDS for q in ("energy", "power")]
CASES = [("edges", t) for t in TABLES] + [(f, t) for f in ("z5", "tiny", "aligned") for t in ("proc_power", "pod_energy")]
# the group pattern's n_groups in the contract test: with PHI5 and PHI1 they land in every regime
PATTERN_GROUPS = {"one": 1, "mod": 63, "random": 7, "node": 1000}


def test_the_shapes_cross_every_regime():
    assert regime(1, 1) == (32, "lds") and regime(1, 8) == (4, "lds") and regime(7, 1)[0] == 8
    assert regime(31, 1) == (2, "lds") and regime(32, 1) == (1, "lds") and regime(4, 8) == (1, "lds")
    assert regime(64, 1) == (1, "lds") and regime(8, 8) == (1, "lds")
    assert regime(65, 1) == (0, "global") and regime(13, 5) == (0, "global")
    assert regime(65536, 1) == (0, "global") and regime(8192, 8) == (0, "global") and regime(1000, 3) == (0, "global")
    assert 8192 * 8 == accel.KACC_QUANT_MAX_QUERIES == 65536
    for s in ((1, 1), (1, 8), (65536, 1), (8192, 8), (31, 1), (32, 1), (64, 1), (65, 1)):
        assert s in SHAPES
    assert {regime(g, len(p))[1] for g in PATTERN_GROUPS.values() for p in (PHI5, PHI1)} == {"lds", "global"}
    assert regime(PATTERN_GROUPS["random"], 5) == (1, "lds") and regime(PATTERN_GROUPS["one"], 5)[0] > 1


@pytest.fixture(scope="module", autouse=True)
def gpu_ready():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    accel.load()
    torch.cuda.set_stream(torch.cuda.Stream())  # every call below runs on a non-default stream


class Outputs:
    """Device outputs of one call, prefilled with the sentinel."""

    def __init__(self, n_groups, n_phi):
        i64 = lambda m: torch.full((m,), SENT64, dtype=torch.int64, device="cuda")  # noqa: E731
        self.G, self.P = n_groups, n_phi
        self.count, self.nan = i64(n_groups), i64(n_groups)
        self.lo, self.hi, self.weight, self.value = (i64(n_groups * n_phi) for _ in range(4))

    def ptrs(self, only=None, skip=None):
        return [getattr(self, n).data_ptr() if (only is None or n == only) and n != skip else 0 for n in OUT_NAMES]

    def host(self):
        """count, nan [G]; lo, hi, weight BITS, value BITS [G, P] — all u64."""
        u64 = lambda t: t.cpu().numpy().view(np.uint64)  # noqa: E731
        return (u64(self.count), u64(self.nan), *(u64(getattr(self, n)).reshape(self.G, self.P) for n in OUT_NAMES[2:]))


def run_quant(acc, table, zone, rows, group, n_groups, phi, stream, mask=None, only=None, skip=None):
    o = Outputs(n_groups, len(phi))
    # a batch without rows still passes an array: a NULL group means "one group" to the call
    o.group = dev_u32(group if group.size else np.zeros(1)) if group is not None else None
    o.mask = dev_u32(mask) if mask is not None else None
    acc.group_quantiles(table, zone, rows, o.group.data_ptr() if group is not None else 0, n_groups, phi,
                        o.mask.data_ptr() if mask is not None else 0, *o.ptrs(only, skip), stream)
    return o


def reference(state, table, L, zone, a, group, n_groups, phi, mask=None, status=None):
    """The contract's outputs (weight and value as bits)."""
    kind = table.split("_")[0]
    st = a["node_status"] if status is None else status
    c, n, lo, hi, w, v = group_quantiles(state[table], table.endswith("power"), L.zones, zone, a[f"{kind}_off"],
                                         a[f"{kind}_slot"], st, mask, group, n_groups, phi)
    bits = lambda x: np.ascontiguousarray(x).view(np.uint64)  # noqa: E731
    return c, n, lo, hi, bits(w), bits(v)


def check(got, want, msg):
    for name, g, w in zip(OUT_NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{msg} {name}"
        np.testing.assert_array_equal(g, w, err_msg=f"{msg} {name}")


def expect_erange(acc, stream):
    with pytest.raises(accel.AccelError) as e:
        acc.sync(stream)
    assert e.value.code == accel.KACC_ERANGE
    assert "bits 0x8000" in str(e.value) and "32768=quantiles" in str(e.value)
    assert "16384=histogram" in str(e.value)  # the earlier names of the message stay


@pytest.mark.parametrize("name,table", CASES)
def test_quantiles_equal_the_contract_over_the_oracle(name, table):
    L, sim, acc = make(name)
    ora = Oracle(L.zones, **L.capacities())
    s = current_stream_handle()
    rng = np.random.default_rng(17)
    kind = table.split("_")[0]
    ranked = interpolated = 0
    for it in range(3):
        a = sim.next_interval()
        t = to_device(a)
        acc.run_interval(interval_from_tensors(t, L.sizes()), s)
        ora.interval(a, L.sizes())
        rows = top_rows_from_tensors(t, KINDS[kind])
        for zone in sorted({0, L.zones - 1}):
            for pattern, n_groups in PATTERN_GROUPS.items():
                group = None if pattern == "one" else group_ids(pattern, a[f"{kind}_off"], n_groups, rng)
                for phi in (PHI5, PHI1):
                    o = run_quant(acc, table, zone, rows, group, n_groups, phi, s)
                    acc.sync(s)  # nothing raised
                    want = reference(ora.state, table, L, zone, a, group, n_groups, phi)
                    check(o.host(), want, f"{name} {table} it{it} z{zone} {pattern} P{len(phi)}")
                    # on the reference, so that the comparison is not vacuous
                    ranked = max(ranked, int(want[0].max()))
                    interpolated += int(((want[2] != want[3]) & (want[4] != 0)).sum())
    if a[f"{kind}_slot"].size > 3:  # the 3-process node has no pod
        assert ranked > 2 and interpolated > 0
    acc.close()


def test_shapes_across_every_regime():
    L, sim, acc = make("edges", seed=5)
    a, t, ora, s = run_intervals(L, sim, acc, 2)
    rng = np.random.default_rng(4)
    for table in ("proc_power", "pod_energy"):
        kind = table.split("_")[0]
        rows = top_rows_from_tensors(t, KINDS[kind])
        for i, (n_groups, n_phi) in enumerate(SHAPES):
            phi = PHI8[:n_phi]
            group = None if n_groups == 1 else group_ids(("mod", "random", "node")[i % 3], a[f"{kind}_off"], n_groups, rng)
            o = run_quant(acc, table, 0, rows, group, n_groups, phi, s)
            acc.sync(s)
            want = reference(ora.state, table, L, 0, a, group, n_groups, phi)
            assert want[0].sum() > 0
            check(o.host(), want, f"shape {table} G{n_groups} P{n_phi}")
    acc.close()


def f64_bits(*v):
    return np.array(v, dtype=np.float64).view(np.uint64)


def crafted_groups(is_power):
    """name -> the value bits of one group's rows; each makes one step of the select decide alone."""
    u64 = lambda *v: np.array(v, dtype=np.uint64)  # noqa: E731
    if not is_power:
        return {
            "equal": u64(*[5] * 9),
            "low byte": np.uint64(0x0123456789ABCD00) + np.arange(40, dtype=np.uint64),
            "high byte": np.arange(0, 256, 7, dtype=np.uint64) << np.uint64(56),
            "halves": u64(1, 2, 3, 4, (1 << 63) + 1, (1 << 63) + 2, (1 << 63) + 3, (1 << 63) + 4),
            "aaab": u64(77, 77, 77, 1 << 40),
            "ends": u64(0, 0, 2 ** 64 - 1, 2 ** 64 - 1),
            "one row": u64(123456789),
        }
    nans = u64(0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF)
    return {
        "equal": f64_bits(*[3.5] * 9),
        "low byte": f64_bits(1.0)[0] + np.arange(40, dtype=np.uint64),
        "high byte": f64_bits(-1e300, -1e200, -1e-300, 1e-300, 1e-200, 1.0, 1e200, 1e300, -1.0, 5e-324, -1e100, 1e100),
        "halves": f64_bits(-4.0, -3.0, -2.0, -1.0, 1.0, 2.0, 3.0, 4.0),
        "aaab": f64_bits(2.5, 2.5, 2.5, 1e9),
        "zeros": f64_bits(-0.0, 0.0, -0.0, 0.0, -0.0),
        "inf ends": f64_bits(-np.inf, -np.inf, 1.0, np.inf, np.inf),
        "inf pair": f64_bits(-np.inf, np.inf),
        "all nan": nans,
        "one row": f64_bits(7.25),
    }


@pytest.mark.parametrize("table", ["pod_power", "pod_energy", "proc_energy"])
def test_crafted_keys(table):
    """Values uploaded into the slots of the batch's rows; the last group stays empty."""
    L, sim, acc = make("edges", seed=11, read_error_frac=0.0)
    a, t, _, s = run_intervals(L, sim, acc, 1, oracle=False)
    kind, is_power = table.split("_")[0], table.endswith("power")
    Z = L.zones
    zone = Z - 1
    crafted = crafted_groups(is_power)
    names = list(crafted)
    words = a[f"{kind}_slot"]
    slots = (words & np.uint32(accel.KACC_SLOT_MASK)).astype(np.int64)
    need = sum(v.size for v in crafted.values())
    assert np.unique(slots).size == slots.size >= need
    rng = np.random.default_rng(6)
    pick = rng.permutation(slots.size)[:need]  # the crafted rows, anywhere in the batch
    group = np.full(slots.size, NONE, dtype=np.uint32)
    tab = acc.download(table).view(np.uint64).reshape(-1, Z)
    at = 0
    for g, name in enumerate(names):
        r = pick[at:at + crafted[name].size]
        at += r.size
        group[r] = g
        tab[slots[r], zone] = crafted[name]
    acc.upload(table, tab.reshape(-1).view(np.float64 if is_power else np.uint64))
    state = {table: acc.download(table)}
    rows = top_rows_from_tensors(t, KINDS[kind])
    phi = [0.0, 0.5, 0.75, 1.0 / 3.0, 1.0]
    for n_groups in (len(names) + 1, 40):  # LDS counters, global counters
        assert regime(n_groups, len(phi))[1] == ("lds" if n_groups < 13 else "global")
        o = run_quant(acc, table, zone, rows, group, n_groups, phi, s)
        acc.sync(s)
        got = o.host()
        check(got, reference(state, table, L, zone, a, group, n_groups, phi), f"crafted {table} G{n_groups}")
        count, nan, lo, hi, weight, value = got
        G = {name: g for g, name in enumerate(names)}
        np.testing.assert_array_equal(count[:len(names)],
                                      [0 if n == "all nan" else crafted[n].size for n in names])
        # the empty group
        assert count[len(names)] == 0 and not lo[len(names)].any() and not weight[len(names)].any()
        assert (value[len(names)] == EMPTY_NAN).all()
        assert (lo[G["equal"]] == crafted["equal"][0]).all() and (hi[G["equal"]] == crafted["equal"][0]).all()
        assert lo[G["low byte"], 0] == crafted["low byte"][0] and lo[G["low byte"], 4] == crafted["low byte"][-1]
        assert hi[G["low byte"], 1] == lo[G["low byte"], 1] + 1  # rank 19.5
        # phi 0.5 of the halves: the lower key ends one top digit, the upper key starts another
        assert lo[G["halves"], 1] == crafted["halves"][3] and hi[G["halves"], 1] == crafted["halves"][4]
        # [a, a, a, b]: phi 0.5 and 1/3 stay on a, phi 0.75 steps from a to b
        x, y = crafted["aaab"][0], crafted["aaab"][3]
        assert (lo[G["aaab"], 1], hi[G["aaab"], 1]) == (x, x) and (lo[G["aaab"], 3], hi[G["aaab"], 3]) == (x, x)
        assert (lo[G["aaab"], 2], hi[G["aaab"], 2]) == (x, y) and (lo[G["aaab"], 4], hi[G["aaab"], 4]) == (y, y)
        assert lo[G["one row"], 2] == hi[G["one row"], 2] == crafted["one row"][0]
        if is_power:
            assert not lo[G["zeros"]].any() and not hi[G["zeros"]].any() and not value[G["zeros"]].any()  # all +0.0
            assert nan[G["all nan"]] == 4 and (value[G["all nan"]] == EMPTY_NAN).all()
            v = value.view(np.float64)
            # -Inf * 1 + -Inf * 0, +Inf * 1 + +Inf * 0, -Inf * 0.5 + Inf * 0.5: the formula's NaN
            assert np.isnan(v[G["inf ends"], 0]) and np.isnan(v[G["inf ends"], 4]) and np.isnan(v[G["inf pair"], 1])
            assert weight[G["inf ends"], 0] == 0 and weight[G["inf ends"], 4] == 0
            assert lo[G["inf ends"], 0] == f64_bits(-np.inf)[0] and lo[G["inf ends"], 4] == f64_bits(np.inf)[0]
        else:
            assert lo[G["ends"], 0] == 0 and lo[G["ends"], 4] == 2 ** 64 - 1 and hi[G["ends"], 1] == 2 ** 64 - 1
    acc.close()


def test_node_mask_and_read_errors():
    """Every third node listed, its complement, none, mask words with other bits, and a node flagged
    with a read error: the contract on the listed rows only."""
    L, sim, acc = make("edges", seed=5)
    a, t, ora, s = run_intervals(L, sim, acc, 2)
    rng = np.random.default_rng(3)
    third = (np.arange(L.n_nodes) % 3 == 0).astype(np.uint32)
    for table, n_groups, phi in (("proc_power", 63, PHI5), ("pod_energy", 7, PHI1), ("proc_energy", 1, PHI5)):
        kind = table.split("_")[0]
        rows = top_rows_from_tensors(t, KINDS[kind])
        group = None if n_groups == 1 else group_ids("random", a[f"{kind}_off"], n_groups, rng)
        got = {}
        for label, mask in (("third", third), ("rest", 1 - third), ("none", np.zeros_like(third)),
                            ("high bit", third * 0x80000000), ("other", third * 7), ("all", None)):
            o = run_quant(acc, table, 0, rows, group, n_groups, phi, s, mask=mask)
            acc.sync(s)
            got[label] = o.host()
            check(got[label], reference(ora.state, table, L, 0, a, group, n_groups, phi, mask=mask),
                  f"mask {label} {table}")
        assert got["none"][0].sum() == 0 and (got["none"][5] == EMPTY_NAN).all() and got["all"][0].sum() > 0
        check(got["high bit"], got["third"], "any nonzero mask word lists")
        check(got["other"], got["third"], "any nonzero mask word lists")
        np.testing.assert_array_equal(got["third"][0] + got["rest"][0], got["all"][0])
        # the largest node flagged with a read error
        status = np.asarray(a["node_status"], dtype=np.uint32).copy()
        status[L.n_nodes - 1] |= accel.KACC_NODE_READ_ERROR
        flagged = dict(t)
        flagged["node_status"] = dev_u32(status)
        o = run_quant(acc, table, 0, top_rows_from_tensors(flagged, KINDS[kind]), group, n_groups, phi, s)
        acc.sync(s)
        want = reference(ora.state, table, L, 0, a, group, n_groups, phi, status=status)
        assert want[0].sum() < got["all"][0].sum() or a["node_status"][L.n_nodes - 1] & accel.KACC_NODE_READ_ERROR
        check(o.host(), want, f"read error {table}")
    acc.close()


def test_bad_ids_slots_and_ranges_are_left_out_and_reported():
    """An id equal to n_groups, a slot word past the capacity, a node whose row range leaves the
    batch: each is left out, every other word stays exact and kacc_sync raises KACC_ERANGE with
    the quantiles bit; KACC_GROUP_NONE raises nothing."""
    L, sim, acc = make("z5", seed=9, read_error_frac=0.0)
    a, t, ora, s = run_intervals(L, sim, acc, 1)
    rng = np.random.default_rng(2)
    n_rows = a["proc_slot"].size
    for n_groups, phi in ((7, PHI5), (63, PHI5)):
        good = group_ids("random", a["proc_off"], n_groups, rng, none_frac=0.0)
        rows = top_rows_from_tensors(t, accel.KACC_KIND_PROC)
        ref = lambda b, g, **kw: reference(ora.state, "proc_energy", L, 0, b, g, n_groups, phi, **kw)  # noqa: E731
        # the id alone
        group = good.copy()
        group[1234] = n_groups
        o = run_quant(acc, "proc_energy", 0, rows, group, n_groups, phi, s)
        expect_erange(acc, s)
        want = ref(a, group)
        assert want[0].sum() == n_rows - 1
        check(o.host(), want, "id == n_groups")
        # KACC_GROUP_NONE in its place: silent
        group[1234] = NONE
        o = run_quant(acc, "proc_energy", 0, rows, group, n_groups, phi, s)
        acc.sync(s)
        check(o.host(), want, "KACC_GROUP_NONE")
        # the slot
        bad = dict(t)
        words = a["proc_slot"].copy()
        words[701] = 0xFFFFFFFF
        bad["proc_slot"] = dev_u32(words)
        o = run_quant(acc, "proc_energy", 0, top_rows_from_tensors(bad, accel.KACC_KIND_PROC), good, n_groups, phi, s)
        expect_erange(acc, s)
        b = dict(a)
        b["proc_slot"] = words
        want = ref(b, good)
        assert want[0].sum() == n_rows - 1
        check(o.host(), want, "slot past the capacity")
        # the row range: n_rows short of the last node's range (nodes 0 and 1 own rows [0, 1000))
        short = top_rows_from_tensors(t, accel.KACC_KIND_PROC)
        short.n_rows = 1000
        o = run_quant(acc, "proc_energy", 0, short, good, n_groups, phi, s)
        expect_erange(acc, s)
        want = ref(a, good, status=np.array([0, 0, accel.KACC_NODE_READ_ERROR], dtype=np.uint32))
        assert 0 < want[0].sum() <= 1000
        check(o.host(), want, "short n_rows")
        # and the next correct call is right and raises nothing
        o = run_quant(acc, "proc_energy", 0, rows, good, n_groups, phi, s)
        acc.sync(s)
        check(o.host(), ref(a, good), "after the clamp")
    acc.close()


def test_each_output_alone_and_each_output_left_out():
    """Every output alone (the others NULL) and every output NULL (the others given) hold the words
    of the full call; a NULL output's neighbours are untouched."""
    L, sim, acc = make("z5", seed=3)
    a, t, ora, s = run_intervals(L, sim, acc, 2)
    rows = top_rows_from_tensors(t, accel.KACC_KIND_PROC)
    rng = np.random.default_rng(1)
    for n_groups, phi in ((7, PHI5), (63, PHI5)):
        group = group_ids("random", a["proc_off"], n_groups, rng)
        want = reference(ora.state, "proc_power", L, 4, a, group, n_groups, phi)
        assert want[0].sum() > 0
        for name in OUT_NAMES:
            for kw in ({"only": name}, {"skip": name}):
                o = run_quant(acc, "proc_power", 4, rows, group, n_groups, phi, s, **kw)
                acc.sync(s)
                for other, g, w in zip(OUT_NAMES, o.host(), want):
                    if (other == name) == ("only" in kw):
                        np.testing.assert_array_equal(g, w, err_msg=f"{other} with {kw}")
                    else:
                        assert np.all(g == SENT64)
    acc.close()


def test_consistent_with_top_fleet_group_sums_and_group_hist():
    L, sim, acc = make("edges", seed=5)
    a, t, ora, s = run_intervals(L, sim, acc, 2)
    rows = top_rows_from_tensors(t, accel.KACC_KIND_PROC)
    rng = np.random.default_rng(12)
    # phi = 1 of the one group is the fleet's top row
    o = run_quant(acc, "proc_power", 0, rows, None, 1, [1.0], s)
    top_count = torch.zeros(1, dtype=torch.int32, device="cuda")
    top_row = torch.zeros(1, dtype=torch.int32, device="cuda")
    top_value = torch.zeros(1, dtype=torch.int64, device="cuda")
    acc.top_fleet("proc_power", 0, 1, rows, top_count.data_ptr(), top_row.data_ptr(), 0, 0, top_value.data_ptr(), s)
    acc.sync(s)
    count, nan, lo, hi, _, value = o.host()
    assert count[0] > 0 and int(top_count[0]) == 1
    top = top_value.cpu().numpy().view(np.uint64)[0]
    assert lo[0, 0] == hi[0, 0] == value[0, 0] == top
    # the rows of a group: ranked + NaN = kacc_group_sums' count
    n_groups = 3
    group = group_ids("random", a["proc_off"], n_groups, rng)
    o = run_quant(acc, "proc_power", 0, rows, group, n_groups, PHI5, s)
    sums = run_group(acc, "proc", rows, group, n_groups, s)
    acc.sync(s)
    count, nan, lo, _, _, _ = o.host()
    np.testing.assert_array_equal(count + nan, sums.host()[0].astype(np.uint64))
    # a group's lower values as the bounds of kacc_group_hist: the cumulative count at the bound
    # equal to out_lo passes `lower`, the one at the bound before it does not
    for g in range(n_groups):
        n = int(count[g])
        assert n > 5
        bounds = np.unique(lo[g])
        bounds = bounds[np.argsort(bound_keys(bounds, True), kind="stable")]
        h = run_hist(acc, "proc_power", 0, rows, group, n_groups, bounds, s)
        acc.sync(s)
        cum = h.host()[1][g]
        for q, f in enumerate(PHI5):
            lower = int(np.floor(np.float64(f) * np.float64(n - 1)))
            j = int(np.flatnonzero(bounds == lo[g, q])[0])
            assert cum[j] > lower
            assert j == 0 or cum[j - 1] <= lower
    acc.close()


def test_two_calls_a_second_stream_and_another_row_order_give_identical_bytes():
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
    for n_groups, phi in ((1, PHI8), (7, PHI5), (1000, PHI5), (65536, PHI1)):
        group = None if n_groups == 1 else group_ids("random", a["proc_off"], n_groups, rng)
        first = run_quant(acc, "proc_power", 0, rows, group, n_groups, phi, s)
        again = run_quant(acc, "proc_power", 0, rows, group, n_groups, phi, s)
        other_order = run_quant(acc, "proc_power", 0, turned_rows, None if group is None else group[flip], n_groups, phi, s)
        acc.sync(s)
        with torch.cuda.stream(second):
            other = run_quant(acc, "proc_power", 0, rows, group, n_groups, phi, second.cuda_stream)
            acc.sync(second.cuda_stream)
        assert first.host()[0].sum() > 0
        check(again.host(), first.host(), f"again G{n_groups}")
        check(other.host(), first.host(), f"second stream G{n_groups}")
        check(other_order.host(), first.host(), f"reversed rows G{n_groups}")
    acc.close()


def test_host_errors_launch_nothing():
    L, sim, acc = make("tiny")
    a, t, _, s = run_intervals(L, sim, acc, 1, oracle=False)
    rows = top_rows_from_tensors(t, accel.KACC_KIND_PROC)
    o = Outputs(8, 2)
    group = dev_u32(np.zeros(3))
    lib, ctx = acc.lib, acc.ctx
    T = accel.TABLE_INDEX

    def call(table=T["proc_power"], zone=0, r=rows, g=group.data_ptr(), n_groups=8, phi=(0.5, 0.99), n_phi=None,
             out=None, c=ctx):
        f = None if phi is None else np.ascontiguousarray(phi, dtype=np.float64)
        n = (0 if f is None else f.size) if n_phi is None else n_phi
        return lib.kacc_group_quantiles(c, table, zone, r, g, n_groups, None if f is None else f.ctypes.data, n, None,
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
    assert call(phi=None, n_phi=2) == E
    assert call(g=None) == E  # NULL group with n_groups 8
    assert call(table=T["node_power"]) == E
    assert call(table=T["proc_ratio"]) == E
    assert call(table=-1) == E
    assert call(zone=L.zones) == E
    assert call(n_phi=0) == E
    assert call(phi=[0.5] * 9) == E
    assert call(n_groups=0) == E
    assert call(n_groups=accel.KACC_GROUP_MAX + 1) == E
    assert call(n_groups=8193, phi=[0.5] * 8) == E  # 8192 x 8 = KACC_QUANT_MAX_QUERIES
    assert call(n_groups=21846, phi=[0.5] * 3) == E
    for bad in ((np.nan,), (-0.1,), (1.0000001,), (0.5, np.nan), (np.inf,)):
        assert call(phi=bad) == E
    assert call(r=many) == E
    assert call(out=[None] * 6) == E
    acc.sync(s)  # nothing raised
    for got in o.host():  # and nothing written
        assert np.all(got == SENT64)
    # -0.0 is in [0, 1]
    assert call(phi=(-0.0, 1.0)) == accel.KACC_OK
    acc.sync(s)
    # a batch without rows, and one without nodes, are no errors: every group is empty
    empty, none = accel.KaccTopRows(), accel.KaccTopRows()
    empty.n_nodes, empty.n_rows, empty.row_off, empty.slot, empty.node_status = 1, 0, group.data_ptr(), None, None
    none.n_nodes, none.n_rows, none.row_off, none.slot, none.node_status = 0, 0, rows.row_off, None, None
    for r in (empty, none):
        for g, n_groups in ((None, 1), (group.data_ptr(), 8)):
            o = Outputs(n_groups, 2)
            assert call(r=r, g=g, n_groups=n_groups) == accel.KACC_OK
            acc.sync(s)
            got = o.host()
            assert (got[5] == EMPTY_NAN).all()
            for words in got[:5]:
                assert not words.any()
    acc.close()
