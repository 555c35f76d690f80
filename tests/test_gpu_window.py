"""kacc_window_* (energy over a window, summed by group) — MI355X only.

Whole outputs and the whole state, byte for byte, against tests/window_ref.py (the header's contract
in numpy) fed from the oracle's tables and the oracle's slot join.  Every output is prefilled with a
pattern, so a word the call did not write shows.  No tolerance anywhere: every sum is an integer.
"""

import numpy as np
import pytest
import torch

from group_ref import group_sums
from kepler_amd import accel, fleet
from kepler_amd.torch_batch import current_stream_handle, interval_from_tensors, to_device, top_rows_from_tensors
from oracle.oracle import Oracle, OracleSlotMap
from window_ref import WindowRef

pytestmark = pytest.mark.gpu

KINDS = {"proc": accel.KACC_KIND_PROC, "ctr": accel.KACC_KIND_CTR, "vm": accel.KACC_KIND_VM,
         "pod": accel.KACC_KIND_POD}
NONE, NEW, MASK = accel.KACC_GROUP_NONE, accel.KACC_SLOT_NEW, accel.KACC_SLOT_MASK
SENT64 = 0x5A5A5A5A5A5A5A5A  # output pre-fill
SENT32 = 0x5A5A5A5A
N_GROUPS = [1, 7, 1000, 65536]  # NULL ids; replicated LDS bins; one LDS copy; global atomics
OUT_NAMES = ["count", "running", "retired", "retired_count", "total", "row"]
FLEETS = {  # name: (node sizes, Z)
    "edges": ([0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 5000], 4),
    "z5": ([700, 300, 1300], 5),  # any-Z path, word by word
}


@pytest.fixture(scope="module", autouse=True)
def gpu_ready():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    accel.load()
    torch.cuda.set_stream(torch.cuda.Stream())  # every call below runs on a non-default stream


def dev_u32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def group_ids(n_rows, n_groups, rng, none_frac=0.05):
    g = rng.integers(0, n_groups, n_rows).astype(np.uint32)
    g[rng.random(n_rows) < none_frac] = NONE
    return g


def skewed_ids(n_rows, n_groups, rng, pattern):
    """Ids that concentrate in a few groups, so that many of a node's terminated slots share one:
    mod3 - three groups, about 21 of 64 slots each; mod7 - seven groups of about 9, more groups at
    the wave merge's threshold than it has rounds, some above it and some below; skew - groups 0, 1, 2
    with a half, a quarter and an eighth of the rows (the eighth: 8 of 64 on average, on both sides of
    the threshold), the rest spread over all groups."""
    if pattern == "mod3":
        return (np.arange(n_rows) % 3).astype(np.uint32)
    if pattern == "mod7":
        return (np.arange(n_rows) % 7).astype(np.uint32)
    u = rng.random(n_rows)
    g = rng.integers(0, n_groups, n_rows).astype(np.uint32)
    g[u < 0.875] = 2
    g[u < 0.75] = 1
    g[u < 0.5] = 0
    return g


def kernel_constant(name):
    """The value of a `constexpr uint32_t` of kacc_window.hip, read from the source the library is built from."""
    import os
    import re
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kepler_amd", "csrc", "kacc_window.hip")
    return int(re.search(rf"constexpr uint32_t {name} = (\d+);", open(src).read()).group(1))


# the census below describes the kernel as built: its threshold, its rounds, its LDS limit
WAVE_SUM, MERGE_ROUNDS, LDS_WORDS = (kernel_constant(n) for n in ("kWaveSum", "kMergeRounds", "kBigWords"))


def merge_census(ref, slot_off, term_slot, term_count, census):
    """What the retire kernel's rounds of 64 terminated slots meet in this step, from the reference's
    state before it: groups with at least WAVE_SUM slots of a round (summed in the wave), groups with
    fewer (every lane its own add), rounds with both, rounds with more large groups than MERGE_ROUNDS,
    rounds whose every group is large (no lane is left for an add of its own)."""
    for n, c in enumerate(np.asarray(term_count).tolist()):
        b0 = int(slot_off[n])
        for c0 in range(0, c, 64):
            g = ref.slot_group[np.asarray(term_slot[b0 + c0:b0 + min(c0 + 64, c)], dtype=np.int64)]
            counts = np.bincount(g[g < ref.G].astype(np.int64))
            counts = counts[counts > 0]
            large = int((counts >= WAVE_SUM).sum())
            census["large"] += large
            census["small"] += int((counts < WAVE_SUM).sum())
            census["mixed"] += int(large > 0 and (counts < WAVE_SUM).any())
            census["over"] += int(large > MERGE_ROUNDS)
            census["all_large"] += int(large > 0 and large == counts.size)


def read_window(w, rows, n_rows, stream, mask=None):
    """One kacc_window_read into prefilled outputs: the six host arrays, in OUT_NAMES' order."""
    G, Z = w.n_groups, w.zones
    i32 = lambda m: torch.full((m,), SENT32, dtype=torch.int32, device="cuda")  # noqa: E731
    i64 = lambda m: torch.full((m,), SENT64, dtype=torch.int64, device="cuda")  # noqa: E731
    o = dict(count=i32(G), running=i64(G * Z), retired=i64(G * Z), retired_count=i32(G), total=i64(G * Z),
             row=i64(n_rows * Z))
    d_mask = dev_u32(mask) if mask is not None else None
    w.read(rows, d_mask.data_ptr() if mask is not None else 0, *[o[n].data_ptr() for n in OUT_NAMES], stream)
    w.accel.sync(stream)
    return [o[n].cpu().numpy().view(np.uint32) if o[n].dtype == torch.int32
            else o[n].cpu().numpy().view(np.uint64).reshape(-1, Z) for n in OUT_NAMES]


def check(got, want, msg):
    for name, g, w in zip(OUT_NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{msg} {name}: {g.dtype}{g.shape} {w.dtype}{w.shape}"
        np.testing.assert_array_equal(g, w, err_msg=f"{msg} {name}")


def check_state(w, ref, msg):
    base, group = w.download()
    np.testing.assert_array_equal(base, ref.base, err_msg=f"{msg} base")
    np.testing.assert_array_equal(group, ref.slot_group, err_msg=f"{msg} slot_group")


def expect_erange(acc, stream):
    with pytest.raises(accel.AccelError) as e:
        acc.sync(stream)
    assert e.value.code == accel.KACC_ERANGE
    assert "bits 0x2000" in str(e.value) and "8192=group sums" in str(e.value)


class Pipeline:
    """Join (with the oracle's beside it) -> window steps -> interval, one call per interval: the
    device windows of `n_groups` and their references move together."""

    def __init__(self, name, kind, reuse, n_groups=N_GROUPS, read_error_frac=0.05, churn=0.05, seed=31,
                 pattern=None):
        self.pattern = pattern  # None: random ids; else skewed_ids' pattern
        self.census = dict(large=0, small=0, mixed=0, over=0, all_large=0)  # of the windows whose retire adds straight to memory
        sizes, Z = FLEETS[name]
        self.kind, self.p, self.Z = kind, kind, Z
        self.L = L = fleet.make_layout(len(sizes), sizes, Z, seed=seed, vm_frac=0.05)
        self.row_off = getattr(L, f"{kind}_off")
        rows = np.diff(self.row_off.astype(np.int64))
        self.slot_off = np.r_[0, np.cumsum(rows * 5 // 4 + 8)].astype(np.uint32)
        caps = L.capacities()
        caps[f"{kind}_slots"] = self.S = int(self.slot_off[-1])
        self.acc = accel.Accel(Z, **caps)
        self.sm = accel.SlotMap(self.acc, KINDS[kind], self.slot_off)
        if reuse:
            self.sm.set_policy(accel.KACC_JOIN_REUSE_TERMINATED)
        self.ojoin, self.ora = OracleSlotMap(self.slot_off, int(reuse)), Oracle(Z, **caps)
        self.sim = fleet.FleetSim(L, seed=seed, churn=0.0, read_error_frac=read_error_frac)
        if kind == "proc":
            self.keys_sim = (fleet.ProcChurn(L, churn=churn, seed=seed) if reuse  # the production pairing
                             else fleet.KeyedChurn(L.proc_off, seed=seed, churn=churn))
        else:
            self.keys_sim = fleet.KeyedChurn(self.row_off, seed=seed, churn=churn, kind=kind)
        self.n_rows = int(self.row_off[-1])
        self.tk = torch.zeros(self.S, dtype=torch.int64, device="cuda")
        self.ts = torch.zeros(self.S, dtype=torch.int32, device="cuda")
        self.tc = torch.zeros(L.n_nodes, dtype=torch.int32, device="cuda")
        self.span = torch.zeros(2 * L.n_nodes, dtype=torch.int32, device="cuda")
        self.s = current_stream_handle()
        self.rng = np.random.default_rng(seed)
        self.wins = [(accel.Window(self.acc, KINDS[kind], G), WindowRef(self.S, Z, G)) for G in n_groups]

    def energy(self):
        return self.ora.state[f"{self.kind}_energy"]

    def interval(self, flags=0, stale=False):
        """One interval.  stale: the slot words of every skipped node's rows are overwritten with
        KACC_SLOT_NEW | a slot of the node before the steps.  Returns the batch."""
        L, kind = self.L, self.kind
        a = self.sim.next_interval()
        keys = self.keys_sim.next_keys()
        status = a["node_status"]
        rc, want_slots, _, ots, ocnt = self.ojoin.join(self.row_off, keys, status)
        assert rc == 0
        t = to_device(a)
        key_dtype = (np.uint32, np.int32) if kind == "proc" else (np.uint64, np.int64)
        d_keys = torch.from_numpy(keys.astype(key_dtype[0]).view(key_dtype[1])).cuda()
        slot_t = t[f"{kind}_slot"]
        self.sm.join(self.n_rows, t[f"{kind}_off"].data_ptr(), d_keys.data_ptr(), t["node_status"].data_ptr(),
                     slot_t.data_ptr(), self.tk.data_ptr(), self.ts.data_ptr(), self.tc.data_ptr(), self.s,
                     self.span.data_ptr() if kind == "proc" else 0)
        if kind == "proc":
            t["node_proc_span"] = self.span
        words = want_slots.copy()
        self.stale_slots = np.zeros(0, dtype=np.int64)
        if stale:
            off = self.row_off.astype(np.int64)
            for n in np.flatnonzero(status & accel.KACC_NODE_READ_ERROR):
                k = off[n + 1] - off[n]
                words[off[n]:off[n + 1]] = (self.slot_off[n] + np.arange(k)).astype(np.uint32) | np.uint32(NEW)
            skipped = (status[np.repeat(np.arange(L.n_nodes), np.diff(off))] & accel.KACC_NODE_READ_ERROR) != 0
            listed_words = slot_t.cpu().numpy().view(np.uint32)[~skipped]
            np.testing.assert_array_equal(listed_words, want_slots[~skipped])  # the join's words, as the oracle's
            slot_t.copy_(dev_u32(words))
            self.stale_slots = (words[skipped] & MASK).astype(np.int64)
        rows = top_rows_from_tensors(t, KINDS[kind])
        pre = self.energy().copy()  # the tables the retiring slots are read from: before this interval
        ids = {}  # windows of one group count take the same ids
        for w, ref in self.wins:
            if w.n_groups not in ids:
                ids[w.n_groups] = (None if w.n_groups == 1
                                   else group_ids(self.n_rows, w.n_groups, self.rng) if self.pattern is None
                                   else skewed_ids(self.n_rows, w.n_groups, self.rng, self.pattern))
            group = ids[w.n_groups]
            d_group = dev_u32(group) if group is not None else None
            w.step(rows, d_group.data_ptr() if group is not None else 0, flags, self.sm, self.ts.data_ptr(),
                   self.tc.data_ptr(), self.s)
            if w.n_groups * (1 + self.Z) > LDS_WORDS:
                merge_census(ref, self.slot_off, ots, ocnt, self.census)
            ref.step(pre, self.row_off, words, status, group, flags, self.slot_off, ots, ocnt)
        a_ora = dict(a)
        a_ora[f"{kind}_slot"] = want_slots
        self.acc.run_interval(interval_from_tensors(t, L.sizes(), L.fast_flag() if kind == "proc" else 0), self.s)
        self.acc.sync(self.s)
        self.ora.interval(a_ora, L.sizes())
        self.a, self.t, self.rows, self.words, self.status = a, t, rows, words, status
        return a

    def check_reads(self, msg):
        stats = dict(retired=0, row=0)
        for w, ref in self.wins:
            want = ref.read(self.energy(), self.row_off, self.words, self.status)
            check(read_window(w, self.rows, self.n_rows, self.s), want, f"{msg} G{w.n_groups}")
            check_state(w, ref, f"{msg} G{w.n_groups}")
            stats["retired"] += int(want[3].sum())
            stats["row"] += int(np.count_nonzero(want[5]))
            assert not ref.erange
        return stats

    def close(self):
        for w, _ in self.wins:
            w.close()
        self.sm.close()
        self.acc.close()


CASES = [("edges", "proc", False), ("edges", "proc", True), ("z5", "proc", False), ("z5", "proc", True),
         ("edges", "pod", True)]


@pytest.mark.parametrize("name,kind,reuse", CASES, ids=[f"{n}-{k}-{'reuse' if r else 'held'}" for n, k, r in CASES])
def test_pipeline_matches_the_contract_over_the_oracle(name, kind, reuse):
    """Join -> window step -> interval for 6 intervals, mark after interval 2: after every interval
    all six outputs and the downloaded state of four windows (G = 1 with NULL ids, 7, 1000, 65536)."""
    p = Pipeline(name, kind, reuse)
    retired = nonzero_rows = 0
    for it in range(6):
        p.interval()
        stats = p.check_reads(f"{name} {kind} it{it}")
        retired, nonzero_rows = retired + stats["retired"], nonzero_rows + stats["row"]
        if it == 2:
            for w, ref in p.wins:
                w.mark(p.s)
                ref.mark(p.energy())
                check(read_window(w, p.rows, p.n_rows, p.s), ref.read(p.energy(), p.row_off, p.words, p.status),
                      f"{name} {kind} marked G{w.n_groups}")
    # the run is not vacuous
    assert retired > 0 and nonzero_rows > 0
    if reuse:
        assert all(ref.reused > 0 for _, ref in p.wins)  # a slot retired and adopted in one step
    np.testing.assert_array_equal(p.acc.download(f"{kind}_energy"), p.energy())  # the tables the reference read
    p.close()


SKEWED = [("mod3", False), ("mod7", False), ("skew", False), ("skew", True)]


@pytest.mark.parametrize("pattern,reuse", SKEWED, ids=[f"{p}-{'reuse' if r else 'held'}" for p, r in SKEWED])
def test_retire_with_ids_concentrated_in_few_groups(pattern, reuse):
    """More groups than LDS holds (the retire phase adds straight into the window's words) with ids
    that concentrate in a few of them: many of a round's 64 terminated slots share a group, so the
    wave sums run - for groups above and below their threshold, in one round, and with more large
    groups than merge rounds.  Outputs and state byte for byte, as everywhere."""
    p = Pipeline("edges", "proc", reuse, n_groups=[2000, 65536], churn=0.1, pattern=pattern)
    retired = 0
    for it in range(5):
        p.interval()
        retired += p.check_reads(f"{pattern} it{it}")["retired"]
        if it == 1:
            for w, ref in p.wins:
                w.mark(p.s)
                ref.mark(p.energy())
    c = p.census
    assert retired > 0 and c["large"] > 0, c  # a wave sum ran
    if pattern == "mod3":
        assert c["all_large"] > 0, c  # rounds in which every slot is summed in the wave (the big nodes' full rounds)
    if pattern == "mod7":
        assert c["over"] > 0 and c["small"] > 0, c  # large groups left over after the last round
    if pattern == "skew":
        assert c["mixed"] > 0 and c["small"] > c["large"], c  # both kinds in one round
    p.close()


def test_stale_new_words_of_skipped_nodes_are_not_adopted():
    p = Pipeline("edges", "proc", False, n_groups=[1, 7], read_error_frac=0.3)
    p.interval()
    touched = 0
    for it in range(3):
        before = [w.download() for w, _ in p.wins]
        p.interval(stale=True)
        touched += p.stale_slots.size
        for (w, ref), (base0, group0) in zip(p.wins, before):
            base1, group1 = w.download()
            np.testing.assert_array_equal(base1[p.stale_slots], base0[p.stale_slots])
            np.testing.assert_array_equal(group1[p.stale_slots], group0[p.stale_slots])
            check_state(w, ref, f"stale it{it} G{w.n_groups}")
    assert touched > 0  # some node was skipped, and its rows carried the stale words
    p.close()


def test_a_read_straight_after_the_mark_is_zero():
    p = Pipeline("z5", "proc", True, n_groups=[7])
    for _ in range(2):
        p.interval()
    w, ref = p.wins[0]
    w.mark(p.s)
    count, running, _, rcount, total, row = read_window(w, p.rows, p.n_rows, p.s)
    assert count.sum() > 0 and not running.any() and not row.any() and not total.any() and not rcount.any()
    p.close()


@pytest.mark.parametrize("kind", ["proc", "pod"])
def test_assign_all_from_the_start_is_the_group_sum(kind):
    """A window created before the first interval, stepped with KACC_WINDOW_ASSIGN_ALL and never
    marked, no read errors: out_running and out_count are kacc_group_sums' out_energy and out_count."""
    sizes, Z = FLEETS["edges"]
    L = fleet.make_layout(len(sizes), sizes, Z, seed=11, shuffle_slots=True, vm_frac=0.05)
    sim = fleet.FleetSim(L, seed=11, churn=0.05, read_error_frac=0.0)
    acc, ora = accel.Accel(Z, **L.capacities()), Oracle(Z, **L.capacities())
    s = current_stream_handle()
    rng = np.random.default_rng(4)
    n_rows = int(getattr(L, f"{kind}_off")[-1])
    wins = [accel.Window(acc, KINDS[kind], G) for G in (7, 1000, 65536)]
    ids = [group_ids(n_rows, w.n_groups, rng) for w in wins]  # a workload keeps its group
    d_ids = [dev_u32(g) for g in ids]
    nonzero = False
    for it in range(3):
        a = sim.next_interval()
        t = to_device(a)
        rows = top_rows_from_tensors(t, KINDS[kind])
        for w, d in zip(wins, d_ids):
            w.step(rows, d.data_ptr(), accel.KACC_WINDOW_ASSIGN_ALL, stream=s)
        acc.run_interval(interval_from_tensors(t, L.sizes()), s)
        ora.interval(a, L.sizes())
        for w, g, d in zip(wins, ids, d_ids):
            G = w.n_groups
            count, running = read_window(w, rows, n_rows, s)[:2]
            gc = torch.full((G,), SENT32, dtype=torch.int32, device="cuda")
            ge = torch.full((G * Z,), SENT64, dtype=torch.int64, device="cuda")
            acc.group_sums(KINDS[kind], rows, d.data_ptr(), G, 0, gc.data_ptr(), ge.data_ptr(), stream=s)
            acc.sync(s)
            np.testing.assert_array_equal(count, gc.cpu().numpy().view(np.uint32))
            np.testing.assert_array_equal(running, ge.cpu().numpy().view(np.uint64).reshape(G, Z))
            want = group_sums(ora.state[f"{kind}_energy"], ora.state[f"{kind}_power"], Z, a[f"{kind}_off"],
                              a[f"{kind}_slot"], a["node_status"], None, g, G)
            np.testing.assert_array_equal(count, want[0])
            np.testing.assert_array_equal(running, want[1])
            assert count.sum() > 0
            nonzero = nonzero or bool(running.any())  # the first interval is the nodes' first reading: no energy yet
    assert nonzero
    for w in wins:
        w.close()
    acc.close()


def test_the_total_is_the_sum_of_the_intervals_own_increases():
    """A second window on the same context, read and marked every interval: its totals add up, word
    by word mod 2^64, to the first window's total over the whole window."""
    p = Pipeline("edges", "proc", True, n_groups=[7, 7], read_error_frac=0.0)
    (whole, _), (each, _) = p.wins
    acc_total = np.zeros((7, p.Z), dtype=np.uint64)
    for it in range(5):
        p.interval()  # both windows take the same ids
        got = read_window(each, p.rows, p.n_rows, p.s)
        with np.errstate(over="ignore"):
            acc_total += got[4]
        each.mark(p.s)
        if it == 0:  # the whole window starts after interval 0, as the per-interval one did
            whole.mark(p.s)
            acc_total[:] = 0
    total = read_window(whole, p.rows, p.n_rows, p.s)
    np.testing.assert_array_equal(total[4], acc_total)
    assert total[2].any() and total[1].any()  # retired and running parts both in it
    p.close()


def test_a_mask_and_its_complement_add_up():
    p = Pipeline("edges", "proc", False, n_groups=[7, 1000, 65536])
    for _ in range(3):
        p.interval()
    third = (np.arange(p.L.n_nodes) % 3 == 0).astype(np.uint32)
    for w, ref in p.wins:
        got = {}
        for label, mask in (("third", third), ("rest", 1 - third), ("all", None)):
            got[label] = read_window(w, p.rows, p.n_rows, p.s, mask=mask)
            check(got[label], ref.read(p.energy(), p.row_off, p.words, p.status, mask), f"mask {label} G{w.n_groups}")
        with np.errstate(over="ignore"):
            for i in (0, 1, 5):  # count, running, row
                np.testing.assert_array_equal(got["third"][i] + got["rest"][i], got["all"][i])
        for label in ("third", "rest"):  # the retired part is not masked
            np.testing.assert_array_equal(got[label][2], got["all"][2])
            np.testing.assert_array_equal(got[label][3], got["all"][3])
        assert got["third"][0].sum() > 0 and got["rest"][0].sum() > 0
    p.close()


CLAMPED = ["term_slot", "term_count", "row_slot", "group_id", "row_range"]


@pytest.mark.parametrize("what", CLAMPED)
def test_clamped_inputs_raise_erange_and_leave_the_rest_exact(what):
    """One malformed input beside a good batch: KACC_ERANGE with bits 0x2000, the malformed entry
    contributes nothing, every other word is the contract's."""
    p = Pipeline("z5", "proc", False, n_groups=[7], read_error_frac=0.0, churn=0.1)
    for _ in range(2):
        p.interval()
    w, ref = p.wins[0]
    L, s = p.L, p.s
    # the next interval's join, by hand, so that one of its results can be broken before the step
    a = p.sim.next_interval()
    keys = p.keys_sim.next_keys()
    rc, words, _, ots, ocnt = p.ojoin.join(p.row_off, keys, a["node_status"])
    assert rc == 0 and ocnt[2] >= 2
    t = to_device(a)
    d_keys = torch.from_numpy(keys.astype(np.uint32).view(np.int32)).cuda()
    p.sm.join(p.n_rows, t["proc_off"].data_ptr(), d_keys.data_ptr(), t["node_status"].data_ptr(),
              t["proc_slot"].data_ptr(), p.tk.data_ptr(), p.ts.data_ptr(), p.tc.data_ptr(), s, p.span.data_ptr())
    p.acc.sync(s)
    words, ots, ocnt = words.copy(), ots.copy(), ocnt.copy()
    group = group_ids(p.n_rows, 7, np.random.default_rng(9), none_frac=0.0)
    row_off = p.row_off.copy()
    fresh = np.flatnonzero(words & np.uint32(NEW))
    assert fresh.size > 2
    if what == "term_slot":
        ots[int(p.slot_off[2]) + 1] = p.S  # node 2's second terminated slot: one past the capacity
    elif what == "term_count":
        ocnt[2] = int(p.slot_off[3] - p.slot_off[2]) + 1  # node 2's whole list is left out
    elif what == "row_slot":
        words[fresh[1]] = np.uint32(p.S) | np.uint32(NEW)  # a NEW row whose slot is one past the capacity
    elif what == "group_id":
        group[fresh[1]] = 7  # n_groups: neither a group nor KACC_GROUP_NONE
    else:
        row_off[2] = p.n_rows + 5  # node 1's range ends, node 2's starts, outside the batch
    p.ts.copy_(dev_u32(ots))
    p.tc.copy_(dev_u32(ocnt))
    t["proc_slot"].copy_(dev_u32(words))
    t_off = dev_u32(row_off)
    rows = top_rows_from_tensors(t, KINDS["proc"])
    rows.row_off = t_off.data_ptr()
    d_group = dev_u32(group)
    w.step(rows, d_group.data_ptr(), 0, p.sm, p.ts.data_ptr(), p.tc.data_ptr(), s)
    expect_erange(p.acc, s)
    ref.step(p.energy(), row_off, words, a["node_status"], group, 0, p.slot_off, ots, ocnt)
    assert ref.erange
    check_state(w, ref, what)
    # the read of the same rows: the tables are interval 2's still, the malformed rows are left out
    ref.erange = False
    want = ref.read(p.energy(), row_off, words, a["node_status"])
    got = read_window(w, rows, p.n_rows, s) if what not in ("row_slot", "row_range") else None
    if got is None:
        assert ref.erange
        o_row = torch.full((p.n_rows * p.Z,), SENT64, dtype=torch.int64, device="cuda")
        o_cnt = torch.full((7,), SENT32, dtype=torch.int32, device="cuda")
        o_run = torch.full((7 * p.Z,), SENT64, dtype=torch.int64, device="cuda")
        w.read(rows, 0, o_cnt.data_ptr(), o_run.data_ptr(), 0, 0, 0, o_row.data_ptr(), s)
        expect_erange(p.acc, s)
        np.testing.assert_array_equal(o_cnt.cpu().numpy().view(np.uint32), want[0])
        np.testing.assert_array_equal(o_run.cpu().numpy().view(np.uint64).reshape(7, p.Z), want[1])
        np.testing.assert_array_equal(o_row.cpu().numpy().view(np.uint64).reshape(-1, p.Z), want[5])
    else:
        assert not ref.erange
        check(got, want, what)
    assert want[0].sum() > 0
    p.close()


def test_assign_all_relabels_and_resets_no_running_base():
    p = Pipeline("edges", "proc", True, n_groups=[1000])
    for _ in range(3):
        p.interval()
    w, ref = p.wins[0]
    w.mark(p.s)
    ref.mark(p.energy())
    before_base, before_group = w.download()
    p.interval(flags=accel.KACC_WINDOW_ASSIGN_ALL)  # every window of this interval draws fresh ids
    p.check_reads("assign all")
    base, group = w.download()
    listed = (p.status[p.sim.node_of_proc] & accel.KACC_NODE_READ_ERROR) == 0
    old = listed & ((p.words & np.uint32(NEW)) == 0)
    s_old = (p.words[old] & MASK).astype(np.int64)
    assert (group[s_old] != before_group[s_old]).any()  # relabelled ...
    np.testing.assert_array_equal(base[s_old], before_base[s_old])  # ... and no running row's base reset
    s_new = (p.words[listed & ~old] & MASK).astype(np.int64)
    assert s_new.size and not base[s_new].any()
    p.close()


def test_host_errors_launch_nothing():
    p = Pipeline("z5", "proc", False, n_groups=[7, 1])
    p.interval()
    (w7, _), (w1, _) = p.wins
    lib, s = p.acc.lib, p.s
    rows = p.rows
    before = w7.download()
    ids = dev_u32(np.zeros(p.n_rows))
    out = torch.full((7 * p.Z,), SENT64, dtype=torch.int64, device="cuda")
    o = out.data_ptr()
    no_off, no_slot, many = (accel.KaccTopRows() for _ in range(3))
    for r in (no_off, no_slot, many):
        r.n_nodes, r.n_rows, r.row_off, r.slot, r.node_status = (rows.n_nodes, rows.n_rows, rows.row_off, rows.slot,
                                                                 rows.node_status)
    no_off.row_off = None
    no_slot.slot = None
    many.n_nodes = p.L.n_nodes + 1
    other = accel.SlotMap(p.acc, accel.KACC_KIND_CTR, np.array([0, 1], dtype=np.uint32))
    acc2 = accel.Accel(p.Z, nodes=1, proc_slots=4, ctr_slots=1, vm_slots=1, pod_slots=1)
    foreign = accel.SlotMap(acc2, accel.KACC_KIND_PROC, np.array([0, 4], dtype=np.uint32))
    h = accel.c_void_p()
    E = accel.KACC_EINVAL

    def step(w=w7, r=rows, g=ids.data_ptr(), flags=0, m=p.sm.handle, ts=p.ts.data_ptr(), tc=p.tc.data_ptr()):
        return lib.kacc_window_step(w.handle, r, g, flags, m, ts, tc, s)

    def read(r=rows, outs=(None, o, None, None, None, None)):
        return lib.kacc_window_read(w7.handle, r, None, *outs, s)

    assert lib.kacc_window_create(p.acc.ctx, 4, 7, accel.ctypes.byref(h)) == E
    assert lib.kacc_window_create(p.acc.ctx, 0, 0, accel.ctypes.byref(h)) == E
    assert lib.kacc_window_create(p.acc.ctx, 0, accel.KACC_GROUP_MAX + 1, accel.ctypes.byref(h)) == E
    assert lib.kacc_window_create(p.acc.ctx, 0, 7, None) == E
    assert h.value is None
    for r in (None, no_off, no_slot, many):
        assert step(r=r) == E and read(r=r) == E
    assert step(g=None) == E  # n_groups 7
    assert step(flags=2) == E
    assert step(m=None) == E and step(ts=None) == E
    assert step(m=other.handle) == E and step(m=foreign.handle) == E
    assert read(outs=(None,) * 6) == E
    assert lib.kacc_window_download(w7.handle, 0, p.S + 1, None, None) == E
    assert lib.kacc_window_download(w7.handle, p.S, 1, None, None) == E
    p.acc.sync(s)  # nothing raised
    assert (out.cpu().numpy().view(np.uint64) == SENT64).all()  # nothing written
    after = w7.download()
    np.testing.assert_array_equal(after[0], before[0])
    np.testing.assert_array_equal(after[1], before[1])
    # valid corner calls: no terminated lists; a batch without rows; one without nodes
    assert step(w=w1, g=None, m=None, ts=None, tc=None) == accel.KACC_OK
    empty, none = accel.KaccTopRows(), accel.KaccTopRows()
    empty.n_nodes, empty.n_rows, empty.row_off, empty.slot, empty.node_status = 1, 0, ids.data_ptr(), None, None
    none.n_nodes, none.n_rows, none.row_off, none.slot, none.node_status = 0, 0, rows.row_off, None, None
    for r in (empty, none):
        assert step(r=r, m=None, ts=None, tc=None) == accel.KACC_OK
        out.fill_(SENT64)
        assert read(r=r) == accel.KACC_OK
        p.acc.sync(s)
        assert not out.cpu().numpy().any()  # every group's running sum: zero
    other.close()
    foreign.close()
    acc2.close()
    p.close()
