"""Inputs of the tracker rule tests: the scenarios tests/test_gpu_tracker_rules.py runs on the device
and tests/test_tracker_ref.py checks on the CPU (model against the Go heap, and that the inputs
reach the cases they are meant to reach).  Pure numpy.

A scenario is one tracker over a few nodes and a few adds.  Every candidate of every add has a
slot of its own (node n's slots in add order, so a node's terminated list is ascending by slot, as
kacc_slot_join writes it).  Keys are unique unless a node lists them itself (the already-tracked
cases).  tables(a) is what the kind's tables hold when add a runs: the rows of the slots listed by
EARLIER adds are overwritten with other values, so a tracked item that is not a frozen copy shows.
"""

import numpy as np

DERIVED = ("proc", "ctr", "vm")  # power = ratio x the node's ActivePower (kacc_derive.hpp); pods store it


def default_key(slot):
    """Unique per slot; neighbours share the low or the high 32-bit word."""
    return ((slot % 7 + 1) << 32) | (slot // 7 + 1)


class Scenario:
    def __init__(self, name, kind, zones, zone, max_size, min_energy=0, capacity=0, tied=False, seed=1):
        self.name, self.kind, self.zones, self.zone = name, kind, zones, zone
        self.max_size, self.min_energy, self.capacity, self.tied = max_size, min_energy, capacity, tied
        self.seed = seed
        self.specs = []  # per node: per add (target-zone energies, keys or None)

    def node(self, *adds):
        """One node: per add an array of target-zone energies in list order, or (energies, keys)."""
        spec = []
        for a in adds:
            e, k = a if isinstance(a, tuple) else (a, None)
            spec.append((np.asarray(e, dtype=np.uint64), None if k is None else np.asarray(k, dtype=np.uint64)))
        self.specs.append(spec)
        return len(self.specs) - 1

    def empty(self, count=1):
        for _ in range(count):
            self.specs.append([])

    def finish(self):
        N, Z = len(self.specs), self.zones
        self.n_nodes = N
        self.n_adds = max(len(s) for s in self.specs)
        cnt = np.zeros((self.n_adds, N), dtype=np.int64)
        for n, spec in enumerate(self.specs):
            for a, (e, _) in enumerate(spec):
                cnt[a, n] = e.size
        self.count = cnt
        per_node = np.maximum(cnt.sum(axis=0), 1)
        self.slot_off = np.r_[0, np.cumsum(per_node)].astype(np.uint32)
        S = self.n_slots = int(self.slot_off[-1])
        self.node_of = np.repeat(np.arange(N), per_node).astype(np.uint32)
        self.start = self.slot_off[:-1].astype(np.int64)[None, :] + np.r_[np.zeros((1, N), np.int64),
                                                                           np.cumsum(cnt, axis=0)[:-1]]
        rng = np.random.default_rng(self.seed)
        self.key = np.array([default_key(s) for s in range(S)], dtype=np.uint64)
        self.energy = rng.integers(0, 2**63, size=(S, Z), dtype=np.uint64) * 2 + rng.integers(0, 2, size=(S, Z),
                                                                                              dtype=np.uint64)
        self.power = rng.random((S, Z)) * 10.0 ** rng.integers(-3, 9, size=(S, Z))
        self.ratio = rng.random(S)
        for n, spec in enumerate(self.specs):
            for a, (e, k) in enumerate(spec):
                s0 = int(self.start[a, n])
                self.energy[s0:s0 + e.size, self.zone] = e
                if k is not None:
                    self.key[s0:s0 + e.size] = k
        return self

    def listed(self, a):
        """Slots listed by add a (every node)."""
        return np.concatenate([np.arange(self.start[a, n], self.start[a, n] + self.count[a, n])
                               for n in range(self.n_nodes)] + [np.zeros(0, np.int64)]).astype(np.int64)

    def tables(self, a):
        """{table name: values} as add a finds them (the whole tables, logical [slot * Z + z])."""
        rng = np.random.default_rng([self.seed, 77, a])
        e, p, ratio = self.energy.copy(), self.power.copy(), self.ratio.copy()
        old = np.concatenate([self.listed(b) for b in range(a)] + [np.zeros(0, np.int64)])
        if old.size:
            e[old] = rng.integers(0, 2**63, size=(old.size, self.zones), dtype=np.uint64)
            p[old] = rng.random((old.size, self.zones)) * 1e7
            ratio[old] = rng.random(old.size)
        k = self.kind
        t = {f"{k}_energy": e.reshape(-1)}
        if k == "pod":
            t["pod_power"] = p.reshape(-1)
        else:  # every add with another ActivePower: a derived power that is not frozen shows
            t[f"{k}_ratio"] = ratio
            t[f"{k}_node"] = self.node_of
            t["node_active_power"] = rng.random(self.n_nodes * self.zones) * 1e8 + 1.0
            t["node_active_energy"] = np.ones(self.n_nodes * self.zones, dtype=np.uint64)
            t["node_cpu_delta"] = np.ones(self.n_nodes)
        return t

    def host_power(self, t):
        """The kind's power table [S, Z] for tables t, computed on the host (process.go:142)."""
        if self.kind == "pod":
            return t["pod_power"].reshape(-1, self.zones)
        ap = t["node_active_power"].reshape(-1, self.zones)
        return t[f"{self.kind}_ratio"][:, None] * ap[self.node_of]

    def term(self, a):
        """(term_key u64 [S], term_slot u32 [S], term_count u32 [N]) of add a."""
        tk = np.zeros(self.n_slots, dtype=np.uint64)
        ts = np.zeros(self.n_slots, dtype=np.uint32)
        for n in range(self.n_nodes):
            b0, c, s0 = int(self.slot_off[n]), int(self.count[a, n]), int(self.start[a, n])
            ts[b0:b0 + c] = np.arange(s0, s0 + c)
            tk[b0:b0 + c] = self.key[s0:s0 + c]
        return tk, ts, self.count[a].astype(np.uint32)


def _draw(rng, values, size, p=None):
    return rng.choice(np.asarray(values, dtype=np.uint64), size=size, p=p)


KINDS = [("proc", 4, 2), ("ctr", 1, 0), ("vm", 3, 1), ("pod", 5, 3)]  # kind, Z, target zone


def small_ties(kind, zones, zone):
    """max_size 5, energies from {1, 2, 3}, 4 adds of 0 to 12 candidates; an all-zero node; the
    101/102/103 pattern behind three higher items; the already-tracked cases."""
    s = Scenario(f"small-ties-{kind}", kind, zones, zone, 5, tied=True, seed=11)
    rng = np.random.default_rng(11)
    s.empty(2)
    for _ in range(4):
        s.node(*[_draw(rng, [1, 2, 3], int(rng.integers(0, 13))) for _ in range(4)])
    s.empty()
    s.zero_node = s.node([0, 0, 0], [0, 0, 0, 0], [], [0] * 6)  # keeps the first 5, never evicts
    # one of two tied minima is evicted by a later, higher item: the rule keeps the older (101)
    s.pattern_node = s.node(([20, 5, 20, 20], [201, 101, 202, 203]), ([5], [102]), ([9], [103]))
    # already tracked (:90), order-independent cases only: key 303 comes again with a lower energy,
    # key 304 with a higher one, while the tracked copy is not the minimum an add evicts.  (A relisted
    # key whose tracked copy is evicted by the same add is left out: whether Go then admits the new
    # copy depends on its map order, and the device decides it per chunk of the list.)
    s.again_full = s.node(([10, 20, 30, 40, 50], [301, 302, 303, 304, 305]),
                          ([5, 60], [303, 306]), ([100, 70], [304, 307]), ([1000, 15], [303, 308]))
    s.again_open = s.node(([10, 20], [401, 402]), ([99, 15], [401, 403]), ([1, 17], [402, 404]))
    s.node(*[_draw(rng, [1, 2, 3], int(rng.integers(0, 13))) for _ in range(4)])
    s.empty(2)
    return s.finish()


def divergence():
    """The example of include/kepler_accel.h as it stands: max_size 2, three single-item adds."""
    s = Scenario("divergence", "proc", 4, 0, 2, tied=True, seed=12)
    s.empty()
    s.node(([5], [101]), ([5], [102]), ([9], [103]))
    s.empty()
    return s.finish()


def chunk_ties(kind, zones, zone):
    """max_size 100, 4 distinct values, 3 adds of 200 per node: several 64-candidate chunks per add,
    a set larger than one 64-item move block."""
    s = Scenario(f"chunk-ties-{kind}", kind, zones, zone, 100, tied=True, seed=13)
    rng = np.random.default_rng(13)
    for lead in (1, 0, 1, 0):
        s.empty(lead)
        s.node(*[_draw(rng, [10, 20, 30, 40], 200, p=[0.4, 0.3, 0.2, 0.1]) for _ in range(3)])
    s.empty()
    return s.finish()


def big_sets(kind, zones, zone, tied):
    """max_size 1500, 6 adds of 300: the set passes 512 (the rank search's LDS copy) inside the second
    add, fills, then evicts.  One more node grows by 90 per add and passes 512 in the last add."""
    s = Scenario(f"big-{'tied' if tied else 'untied'}-{kind}", kind, zones, zone, 1500, tied=tied, seed=14)
    rng = np.random.default_rng(14 + tied)
    distinct = (10**6 + rng.permutation(2 * 1800 + 540).astype(np.uint64) * 3).tolist()

    def draw(c):
        if tied:
            return _draw(rng, [3, 5, 8, 13, 21, 34, 55, 89], c)
        return [distinct.pop() for _ in range(c)]

    s.empty()
    s.node(*[draw(300) for _ in range(6)])
    s.empty()
    s.node(*[draw(90) for _ in range(6)])
    s.node(*[draw(300) for _ in range(6)])
    s.empty()
    return s.finish()


def max_bounded():
    """One node at KACC_TRACKER_MAX_BOUNDED: max_size 8192, 3 adds of 4000, about 50 values."""
    s = Scenario("max-bounded", "proc", 4, 0, 8192, tied=True, seed=15)
    rng = np.random.default_rng(15)
    s.node(*[_draw(rng, np.arange(1, 51) * 7, 4000) for _ in range(3)])
    return s.finish()


def threshold(m=1000):
    """min_energy m: exactly m is kept, m - 1 is dropped."""
    s = Scenario("threshold", "proc", 4, 0, 5, min_energy=m, seed=16)
    s.empty()
    s.node([m, m - 1, m + 1, 0], [m - 1, m, 2 * m])
    s.empty()
    return s.finish()


def overflow():
    """Unlimited, capacity 100: node 1 receives 60 + 60 and overflows; node 2 stays under the
    capacity, node 4 reaches it exactly."""
    s = Scenario("overflow", "proc", 4, 0, -1, capacity=100, seed=17)
    rng = np.random.default_rng(17)
    s.empty()
    s.over_node = s.node(_draw(rng, np.arange(1, 30), 60), _draw(rng, np.arange(1, 30), 60))
    s.node(_draw(rng, np.arange(1, 30), 50), _draw(rng, np.arange(1, 30), 40))
    s.empty()
    s.node(_draw(rng, np.arange(1, 30), 30), _draw(rng, np.arange(1, 30), 70))
    return s.finish()


def after_overflow():
    """The add that follows the overflow and a clear, on the same tracker: under the capacity."""
    s = Scenario("after-overflow", "proc", 4, 0, -1, capacity=100, seed=18)
    rng = np.random.default_rng(18)
    s.empty()
    for c in (70, 100, 1, 30):
        s.node(_draw(rng, np.arange(1, 30), c))
    return s.finish()


def gpu_scenarios():
    """Every scenario of tests/test_gpu_tracker_rules.py that is compared with the model node by node."""
    out = [small_ties(*k) for k in KINDS]
    out += [divergence(), chunk_ties("proc", 4, 2), chunk_ties("pod", 5, 3)]
    out += [big_sets("pod", 5, 3, True), big_sets("proc", 4, 0, False), big_sets("vm", 3, 1, True),
            big_sets("pod", 5, 0, False)]
    out += [max_bounded(), threshold(), overflow(), after_overflow()]
    return out
