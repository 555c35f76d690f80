"""The slot join's tables themselves, read back after every call — MI355X only.

test_gpu_join.py sees slot words only; a key in a wrong group, a stale slot after a cuckoo
kick or a leftover duplicate shows there an interval later or never.  Here every call is
compared with the oracle as there (slot words, terminated list, span) AND every processed
node's table (kacc_debug_slotmap_node) must hold exactly the oracle's live IDs where the
table rules put them (tests/join_model.py: check_table; test_join_model.py shows that check
failing on corrupted tables).  The shapes are the ones that reach what test_gpu_join.py's
never do: the kick loop of step 6 (forced with PID lists found on the CPU, where single-key
inserts make the model exact bucket for bucket), its homeless exit, full nodes, a new ID
given twice across waves / windows / among the deferred keys, long churn and wrapping probe
chains of the 64-bit kinds, join_big<uint64_t>.  Everything is an integer, compared exactly.
"""

import ctypes

import numpy as np
import pytest
import torch

import join_cases as jc
import join_model as jm
from kepler_amd import accel, fleet
from kepler_amd.torch_batch import current_stream_handle
from oracle.oracle import OracleSlotMap

pytestmark = pytest.mark.gpu

PROC, CTR, POD = accel.KACC_KIND_PROC, accel.KACC_KIND_CTR, accel.KACC_KIND_POD
REUSE = accel.KACC_JOIN_REUSE_TERMINATED
MASK, NEW = 0x7FFFFFFF, 0x80000000
POLICIES = pytest.mark.parametrize("policy", [0, REUSE], ids=["held", "reuse"])


@pytest.fixture(scope="module", autouse=True)
def gpu_ready():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    accel.load()
    torch.cuda.set_stream(torch.cuda.Stream())


@pytest.fixture(params=[-1, 90623], ids=["production", "cuckoo-shift"])
def join_variant(request):
    """The production join and the same kernel without the uniform map's early table loads
    (same hashes, same tables), set for the maps the test creates (read at reset)."""
    lib = accel.load()
    lib.kacc_debug_set_join_variant.argtypes = [ctypes.c_int]
    lib.kacc_debug_set_join_variant.restype = ctypes.c_int
    prev = lib.kacc_debug_set_join_variant(request.param)
    yield request.param
    lib.kacc_debug_set_join_variant(prev)


def offsets(sizes):
    return np.r_[0, np.cumsum(sizes)].astype(np.uint32)


class Harness:
    """A device slot map, the oracle's, and the oracle's live IDs per node."""

    def __init__(self, kind, slot_off, policy=0, cuckoo=True):
        # cuckoo: the small PID tables are the production format (False: an earlier linear one)
        self.kind, self.policy, self.cuckoo = kind, policy, cuckoo
        self.slot_off = np.asarray(slot_off, dtype=np.uint32)
        self.N = self.slot_off.size - 1
        self.open_device()
        self.forget()

    def forget(self):
        self.ora = OracleSlotMap(self.slot_off, self.policy)
        self.live = [dict() for _ in range(self.N)]

    def reset(self):
        self.m.reset()
        self.forget()

    # ---- the device (everything that touches it is in these three methods) ---------------
    def open_device(self):
        total = max(int(self.slot_off[-1]), 1)
        caps = dict(nodes=self.N, proc_slots=1, ctr_slots=1, vm_slots=1, pod_slots=1)
        caps[{PROC: "proc_slots", CTR: "ctr_slots", POD: "pod_slots"}[self.kind]] = total
        self.acc = accel.Accel(1, **caps)
        self.m = accel.SlotMap(self.acc, self.kind, self.slot_off)
        if self.policy:
            self.m.set_policy(self.policy)
        self.tk = torch.zeros(total, dtype=torch.int64, device="cuda")
        self.ts = torch.zeros(total, dtype=torch.int32, device="cuda")
        self.cnt = torch.zeros(self.N, dtype=torch.int32, device="cuda")
        self.span = torch.zeros(2 * self.N, dtype=torch.int32, device="cuda")
        fn = self.acc.lib.kacc_debug_slotmap_node
        fn.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32] + [ctypes.c_void_p] * 3
        fn.restype = ctypes.c_int

    def device_join(self, row_off, keys, status=None):
        """-> (0 or the error code of the sync, slot words, counts, term keys, term slots, spans)"""
        n_rows = int(row_off[-1])
        d_off = torch.from_numpy(row_off.astype(np.int32)).cuda()
        if self.kind == PROC:  # PIDs are u32 keys
            d_keys = torch.from_numpy(keys.astype(np.uint32).view(np.int32)).cuda()
        else:
            d_keys = torch.from_numpy(keys.astype(np.uint64).view(np.int64)).cuda()
        d_st = None if status is None else torch.from_numpy(status.astype(np.int32)).cuda()
        out = torch.zeros(max(n_rows, 1), dtype=torch.int32, device="cuda")
        s = current_stream_handle()
        self.m.join(n_rows, d_off.data_ptr(), d_keys.data_ptr(), 0 if d_st is None else d_st.data_ptr(),
                    out.data_ptr(), self.tk.data_ptr(), self.ts.data_ptr(), self.cnt.data_ptr(), s,
                    self.span.data_ptr())
        code = 0
        try:
            self.acc.sync(s)
        except accel.AccelError as e:
            code = e.code
        return (code, out[:n_rows].cpu().numpy().view(np.uint32), self.cnt.cpu().numpy().view(np.uint32),
                self.tk.cpu().numpy().view(np.uint64), self.ts.cpu().numpy().view(np.uint32),
                self.span.cpu().numpy().view(np.uint32))

    def dump(self, n):
        """Node n's table: (keys u64 [H], slots u32 [H])."""
        H = jm.node_buckets(int(self.slot_off[n + 1] - self.slot_off[n]))
        key, slot, got_h = np.zeros(H, dtype=np.uint64), np.zeros(H, dtype=np.uint32), ctypes.c_uint32()
        fn = self.acc.lib.kacc_debug_slotmap_node
        assert fn(self.m.handle, n, H, ctypes.addressof(got_h), key.ctypes.data, slot.ctypes.data) == 0
        assert got_h.value == H
        return key, slot

    # ---- checks --------------------------------------------------------------------------
    def fmt(self, n):
        if self.kind != PROC:
            return "linear64"
        small = jm.node_buckets(int(self.slot_off[n + 1] - self.slot_off[n])) <= 4096
        return "cuckoo" if small and self.cuckoo else "linear32"

    def check_node(self, n, row_off, keys, got, want):
        """Node n of a call: the device's outputs against the oracle's, then its table."""
        (_, g_out, g_cnt, g_tk, g_ts, g_span), (_, w_out, w_tk, w_ts, w_cnt) = got, want
        r0, r1, s0 = int(row_off[n]), int(row_off[n + 1]), int(self.slot_off[n])
        np.testing.assert_array_equal(g_out[r0:r1], w_out[r0:r1], err_msg=f"node {n} slot words")
        c = int(w_cnt[n])
        assert int(g_cnt[n]) == c, f"node {n} terminated count"
        np.testing.assert_array_equal(g_tk[s0:s0 + c], w_tk[s0:s0 + c], err_msg=f"node {n} terminated keys")
        np.testing.assert_array_equal(g_ts[s0:s0 + c], w_ts[s0:s0 + c], err_msg=f"node {n} terminated slots")
        w = w_out[r0:r1] & MASK
        span = (int(w.min()), int(w.max())) if w.size else (1, 0)
        assert (int(g_span[2 * n]), int(g_span[2 * n + 1])) == span, f"node {n} span"
        self.live[n] = {int(k): int(x) - s0 for k, x in zip(keys[r0:r1].tolist(), w.tolist())}
        d = self.dump(n)
        jm.check_table(d, self.live[n], self.fmt(n))
        return d

    def step(self, row_off, keys, status=None):
        """One valid call: every processed node against the oracle, every such node's table
        against the rules.  -> (slot words, per-node dumps (None for a skipped node))"""
        row_off, keys = np.asarray(row_off, dtype=np.uint32), np.asarray(keys, dtype=np.uint64)
        want = self.ora.join(row_off, keys, status)
        assert want[0] == 0, "the test's own batch is invalid"
        got = self.device_join(row_off, keys, status)
        assert got[0] == 0, f"device error {got[0]}"
        dumps = [None if status is not None and status[n] else self.check_node(n, row_off, keys, got, want)
                 for n in range(self.N)]
        return got[1], dumps

    def failing_call(self, row_off, keys, healthy):
        """A call that must raise KACC_ERANGE at sync; its `healthy` nodes are served as usual
        (the oracle's words, terminated list and span, and a sound table)."""
        row_off, keys = np.asarray(row_off, dtype=np.uint32), np.asarray(keys, dtype=np.uint64)
        want = self.ora.join(row_off, keys, None)
        got = self.device_join(row_off, keys)
        assert got[0] == accel.KACC_ERANGE
        for n in healthy:
            self.check_node(n, row_off, keys, got, want)


def assert_same_table(dump, model):
    """Bucket for bucket: the same keys, and the same slot under every live key."""
    keys, slots = [int(k) for k in dump[0]], [int(s) for s in dump[1]]
    assert keys == model[0]
    assert [s for k, s in zip(keys, slots) if k != jm.EMPTY] == [s for k, s in zip(*model) if k != jm.EMPTY]


def proc_keys(n, first=300):
    """n distinct node-local PIDs, ascending like /proc."""
    return (first + 3 * np.arange(n)).astype(np.uint64)


class Churn:
    """Exactly `c` rows of each node take a new ID per interval (PIDs past 2^22 or odd 64-bit IDs)."""

    def __init__(self, keys, row_off, seed, wide=False):
        self.keys, self.row_off, self.wide = np.array(keys, dtype=np.uint64), row_off, wide
        self.rng = np.random.default_rng(seed)
        self.next_id = 1 << 22

    def fresh(self, k):
        if self.wide:
            return self.rng.integers(0, 2**62, size=k, dtype=np.int64).astype(np.uint64) * np.uint64(2) + np.uint64(1)
        self.next_id += k
        return np.arange(self.next_id - k, self.next_id, dtype=np.uint64)

    def next_keys(self, counts):
        for n, c in enumerate(counts):
            r0, r1 = int(self.row_off[n]), int(self.row_off[n + 1])
            rows = r0 + self.rng.choice(r1 - r0, size=c, replace=False)
            self.keys[rows] = self.fresh(c)
        return self.keys.copy()


# ---- the debug read itself ------------------------------------------------------------------


def test_dump_rejects_bad_arguments():
    h = Harness(PROC, offsets([jc.SLOTS, 100]))
    fn, got_h = h.acc.lib.kacc_debug_slotmap_node, ctypes.c_uint32()
    key, slot = np.zeros(256, dtype=np.uint64), np.zeros(256, dtype=np.uint32)
    args = ctypes.addressof(got_h), key.ctypes.data, slot.ctypes.data
    assert fn(h.m.handle, 2, 256, *args) == accel.KACC_EINVAL  # two nodes: 0 and 1
    assert fn(h.m.handle, 1, 255, *args) == accel.KACC_EINVAL and got_h.value == 256  # 100 slots: 256 buckets
    assert fn(h.m.handle, 1, 256, None, key.ctypes.data, slot.ctypes.data) == accel.KACC_EINVAL
    assert fn(h.m.handle, 1, 256, *args) == 0 and (key == jm.EMPTY).all()


@pytest.fixture(params=[31, 511], ids=["8-B-packed", "6-B-linear"])
def linear_variant(request):
    """Earlier kernels whose small PID tables probe linearly: packed 8-B entries, and 6-B
    buckets with tombstones: the two storage formats the production tests do not read."""
    lib = accel.load()
    lib.kacc_debug_set_join_variant.argtypes = [ctypes.c_int]
    lib.kacc_debug_set_join_variant.restype = ctypes.c_int
    prev = lib.kacc_debug_set_join_variant(request.param)
    yield request.param
    lib.kacc_debug_set_join_variant(prev)


def test_dump_decodes_linear_pid_formats(linear_variant):
    sizes = [42, 300]
    row_off = offsets(sizes)
    h = Harness(PROC, offsets([int(s * 1.35) + 8 for s in sizes]), cuckoo=False)
    sim = fleet.KeyedChurn(row_off, seed=3, churn=0.1, kind="proc")
    tombs = 0
    for it in range(6):
        _, dumps = h.step(row_off, sim.next_keys())
        tombs += sum(jm.tombstones(d) for d in dumps)
    assert tombs > 0


# ---- a: the invariant under churn ----------------------------------------------------------


@POLICIES
def test_table_invariant_under_churn(policy, join_variant):
    """Seven small nodes (the cuckoo table) and a 3,653-slot node (join_big), 12 intervals at
    10 % churn with read errors: the oracle's words and a sound table after every call."""
    sizes = [0, 1, 5, 42, 64, 300, 2000, 2700]
    slots = [int(s * 1.35) + 8 for s in sizes]
    assert [jm.node_buckets(s) <= 4096 for s in slots] == [True] * 7 + [False] and slots[-1] == 3653
    row_off = offsets(sizes)
    h = Harness(PROC, offsets(slots), policy)
    sim = fleet.KeyedChurn(row_off, seed=31, churn=0.1, kind="proc")
    rng = np.random.default_rng(9)
    for it in range(12):
        keys = sim.next_keys()
        status = None
        if it % 4 == 3:
            status = np.where(rng.random(len(sizes)) < 0.3, accel.KACC_NODE_READ_ERROR, 0).astype(np.uint32)
        h.step(row_off, keys, status)


# ---- b: forced kicks on the smallest table ---------------------------------------------------


def build_one_per_call(h, keys, model, tail=()):
    """Present keys[:1], keys[:2], ... to node 0 (one new key per call: a single lane inserts,
    so the model's table is THE table); `tail`: the other nodes' rows.  -> chain lengths"""
    chains = []
    for i in range(len(keys)):
        row_off = offsets([i + 1] + [len(t) for t in tail])
        batch = np.concatenate([np.array(keys[:i + 1], dtype=np.uint64)] + [np.asarray(t, dtype=np.uint64) for t in tail])
        words, dumps = h.step(row_off, batch)
        assert int(words[i]) == (i | NEW) and not (words[:i] & NEW).any()
        chains.append(jm.place(model, keys[i], i))
        assert_same_table(dumps[0], model)
    return chains


@pytest.mark.parametrize("case", ["single-kick", "long-chain"])
def test_forced_kicks_smallest_table(case, join_variant):
    """One node of 42 slots (64 buckets, 16 groups) built one new key per call from a fixed PID
    list whose last key finds both groups full: placed by one kick, or by a chain of ten
    (test_join_model.py asserts the lists); the table equals the model's after every call."""
    keys, kicks = (jc.SINGLE_KICK, 1) if case == "single-kick" else (jc.LONG_CHAIN, jc.LONG_CHAIN_KICKS)
    h = Harness(PROC, offsets([jc.SLOTS]))
    model = jm.new_table(jc.BUCKETS)
    chains = build_one_per_call(h, keys, model)
    assert chains == [0] * (len(keys) - 1) + [kicks]
    print(f"{case}: last key placed by a chain of {chains[-1]} kicks")
    for _ in range(2):  # every key is found where the kicks left it
        words, dumps = h.step([0, len(keys)], keys)
        assert not (words & NEW).any() and sorted(words.tolist()) == list(range(len(keys)))
        assert_same_table(dumps[0], model)


# ---- c: a forced kick at the production shape ----------------------------------------------


def test_forced_kick_production_shape(join_variant):
    """A full 2,730-slot node on a uniform map (every table 4,096 buckets: production takes the
    early table loads).  The fill is one call (racy placement: the invariant only); then one row
    terminates and the only new row carries a key, found with the model on the table read
    back, whose two groups are both full: the kicks must leave the model's table."""
    S = 2730
    assert jm.node_buckets(S) == 4096
    h = Harness(PROC, offsets([S, S]), REUSE)
    row_off = offsets([S, 100])
    keys = fleet.KeyedChurn(row_off, seed=41, churn=0.0, kind="proc").next_keys()
    _, dumps = h.step(row_off, keys)
    model = ([int(k) for k in dumps[0][0]], [int(s) for s in dumps[0][1]])
    rel = h.live[0][int(keys[0])]  # row 0 terminates; the new row takes its slot (reuse)
    jm.remove(model, int(keys[0]), "cuckoo")
    found = []  # (chain, key, table after): the longest chain of the first 32 such keys is used
    for cand in range(5_000_000, 5_000_000 + (1 << 20)):  # never a PID of the fill
        if not jm.both_full(model, cand):
            continue
        trial = (model[0][:], model[1][:])
        try:
            found.append((jm.place(trial, cand, rel), cand, trial))
        except jm.Homeless:
            continue
        if len(found) == 32:
            break
    assert found, "no key with both groups full among 2^20 candidates"
    chain, cand, model = max(found, key=lambda f: f[0])
    assert chain >= 1
    print(f"production shape: key {cand} placed by a chain of {chain} kicks")
    keys[0] = cand
    words, dumps = h.step(row_off, keys)
    assert int(words[0]) == (rel | NEW) and not (words[1:] & NEW).any()
    assert_same_table(dumps[0], model)
    words, dumps = h.step(row_off, keys)  # and every key is found where the kicks left it
    assert not (words & NEW).any()
    assert_same_table(dumps[0], model)


# ---- d: the homeless key -------------------------------------------------------------------


def test_homeless_key_fails_the_call(join_variant):
    """Nine PIDs that share one pair of groups cannot sit in eight buckets: KACC_ERANGE at sync
    (kepler_accel.h: that node's map is unspecified until reset — the key without a bucket is
    one of the first eight, whatever the order), the call's other node is served as usual, and
    after a reset the map joins exactly."""
    h = Harness(PROC, offsets([jc.SLOTS, 300]))
    row_off = offsets([9, 200])
    keys = np.r_[np.array(jc.CONFINED9, dtype=np.uint64), proc_keys(200)]
    h.failing_call(row_off, keys, healthy=[1])
    h.reset()
    ok = np.r_[np.array(jc.SINGLE_KICK, dtype=np.uint64), proc_keys(200)]
    for _ in range(2):
        h.step(offsets([len(jc.SINGLE_KICK), 200]), ok)


# ---- e: full nodes ---------------------------------------------------------------------------


@POLICIES
def test_full_nodes(policy, join_variant):
    """rows == slots (42 and 2,730: the fullest cuckoo tables there are), 10 intervals with 5 % of
    the rows replaced.  Reuse: every terminated slot is handed out again in the same call.
    Held: rows = slots - replaced rows, so the new rows take exactly the free slots."""
    S = [42, 2730]
    c = [2, 136]
    rows = S if policy else [s - x for s, x in zip(S, c)]
    row_off = offsets(rows)
    h = Harness(PROC, offsets(S), policy)
    sim = Churn(np.r_[proc_keys(rows[0]), proc_keys(rows[1])], row_off, seed=3)
    h.step(row_off, sim.keys)
    for it in range(10):
        words, _ = h.step(row_off, sim.next_keys(c))
        assert [int((words[row_off[n]:row_off[n + 1]] & NEW != 0).sum()) for n in range(2)] == c


# ---- f: a new ID given twice -----------------------------------------------------------------


@pytest.mark.parametrize("second", [200, 1500], ids=["two-waves-one-window", "two-windows"])
def test_new_id_twice_all_new_node(second, join_variant):
    """An all-new node of 2,000 rows (four windows of 512 inserts) with rows 3 and `second`
    carrying one ID: lanes of two waves of the first window, or the first and the third window."""
    h = Harness(PROC, offsets([2708, 413]))
    row_off = offsets([2000, 300])
    keys = np.r_[proc_keys(2000), proc_keys(300)]
    bad = keys.copy()
    bad[second] = bad[3]
    h.failing_call(row_off, bad, healthy=[1])
    h.reset()
    for _ in range(2):
        h.step(row_off, keys)


def test_new_id_twice_among_deferred(join_variant):
    """On the single-kick table short of its last key, two rows carry that key: both find both
    groups full, lane 0 places the first and meets it again for the second."""
    h = Harness(PROC, offsets([jc.SLOTS, 300]))
    tail = proc_keys(200)
    built = jc.SINGLE_KICK[:-1]
    model = jm.new_table(jc.BUCKETS)
    assert build_one_per_call(h, built, model, tail=[tail]) == [0] * len(built)
    assert jm.both_full(model, jc.KICKER)
    keys = np.r_[np.array(built + [jc.KICKER, jc.KICKER], dtype=np.uint64), tail]
    h.failing_call(offsets([len(built) + 2, 200]), keys, healthy=[1])
    h.reset()
    ok = np.r_[np.array(jc.SINGLE_KICK, dtype=np.uint64), tail]
    for _ in range(2):
        h.step(offsets([len(jc.SINGLE_KICK), 200]), ok)


# ---- g: the 64-bit kinds ---------------------------------------------------------------------


def churn_until_rebuild(h, sizes):
    """30 intervals at 10 % churn; some node's tombstone count must fall between two calls
    (its table was rebuilt: check_table has held the 3/4 bound after every call)."""
    row_off = offsets(sizes)
    sim = fleet.KeyedChurn(row_off, seed=13, churn=0.1, kind="ctr")
    before, rebuilds = [0] * len(sizes), 0
    for it in range(30):
        _, dumps = h.step(row_off, sim.next_keys())
        tombs = [jm.tombstones(d) for d in dumps]
        rebuilds += sum(t < b for t, b in zip(tombs, before))
        before = tombs
    assert rebuilds >= 1, "no table was rebuilt in 30 intervals"


@pytest.mark.parametrize("kind", [CTR, POD], ids=["ctr", "pod"])
def test_u64_small_nodes_long_churn(kind, join_variant):
    sizes = [250, 2000, 0, 40]
    slots = [int(s * 1.35) + 8 for s in sizes]
    assert slots[1] == 2708 and jm.node_buckets(slots[1]) == 4096
    churn_until_rebuild(Harness(kind, offsets(slots)), sizes)


@pytest.mark.parametrize("kind", [CTR, POD], ids=["ctr", "pod"])
def test_u64_big_node_long_churn(kind, join_variant):
    """One node of 3,000 rows and 4,058 slots: 8,192 buckets, join_big<uint64_t>."""
    assert jm.node_buckets(4058) == 8192
    churn_until_rebuild(Harness(kind, offsets([4058])), [3000])


def keys_with_home(H, wide, count, skip=0):
    """`count` distinct keys (after the first `skip` such keys) whose home bucket is H - 1 or H - 2."""
    x = np.arange(1, 1 << 22, dtype=np.uint64)
    hb = ((x * np.uint64(0x9E3779B1)) & np.uint64(jm.M32)) >> np.uint64(32 - (H.bit_length() - 1))
    x = x[hb >= H - 2][skip:skip + count]
    assert x.size == count
    if wide:  # the home bucket hashes low ^ high
        hi = np.arange(1, count + 1, dtype=np.uint64) * np.uint64(0x01000193)
        x = (hi << np.uint64(32)) | (x ^ hi)
    assert all(jm.home(int(k), H, wide) >= H - 2 for k in x)
    return x


@pytest.mark.parametrize("kind", [PROC, CTR, POD], ids=["proc", "ctr", "pod"])
def test_probe_chain_wraps_past_the_table_end(kind, join_variant):
    """Twelve IDs whose home bucket is one of the table's last two (their chain wraps to bucket
    0), half of them terminated, six others of the same home buckets inserted: a 42-slot node
    (join_small's linear table for the 64-bit kinds; PIDs have no probe chain there) and a
    2,731-slot node (8,192 buckets, join_big)."""
    S = [42, 2731]
    wide = kind != PROC
    h = Harness(kind, offsets(S))
    assert [jm.node_buckets(s) for s in S] == [64, 8192]
    first = [keys_with_home(jm.node_buckets(s), wide, 12) for s in S]
    other = [keys_with_home(jm.node_buckets(s), wide, 6, skip=12) for s in S]
    if not wide:  # the cuckoo table has no home bucket: plain PIDs
        first[0], other[0] = proc_keys(12), proc_keys(6, first=1000)
    _, dumps = h.step(offsets([12, 12]), np.r_[first[0], first[1]])
    for n in (0, 1):
        if h.fmt(n) != "cuckoo":
            assert sum(int(k) != jm.EMPTY for k in dumps[n][0][:10]) >= 10, "the chain wrapped"
    h.step(offsets([6, 6]), np.r_[first[0][::2], first[1][::2]])
    batch = np.r_[first[0][::2], other[0], first[1][::2], other[1]]
    words, _ = h.step(offsets([12, 12]), batch)
    words, _ = h.step(offsets([12, 12]), batch)
    assert not (words & NEW).any()
