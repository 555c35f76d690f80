"""tests/tracker_ref.py (the documented retention and order rule of kacc_tracker_add) against Go's
container/heap restatement (oracle/kor_tracker.cpp), and the inputs of
tests/test_gpu_tracker_rules.py — CPU.

What the rule guarantees against Go: where no item was ever dropped at the energy of the last item
kept, the retained items are Go's, exactly; with ties at that boundary the retained TARGET-ZONE
ENERGIES are Go's, and the retained IDs are the rule's own choice among energy-equivalent sets
(Go's choice depends on its heap's layout, test_divergence_example).
"""

import numpy as np
import pytest

import tracker_cases
from oracle.oracle import OracleTracker
from tracker_ref import TrackerModel

SCENARIOS = tracker_cases.gpu_scenarios()
KSET_LDS = 512  # kacc_tracker.hip kSetLds: larger sets are searched in global memory


def run_both(s, on_add=None):
    """The scenario through the model and through one Go heap per node; on_add(a, model, oracle)."""
    model = TrackerModel(s.n_nodes, s.zones, s.zone, s.max_size, s.min_energy, s.capacity)
    ora = OracleTracker(s.max_size, s.min_energy, s.zones, s.zone)
    sizes = []
    for a in range(s.n_adds):
        t = s.tables(a)
        e, p = t[f"{s.kind}_energy"], s.host_power(t)
        tk, ts, tc = s.term(a)
        model.add(s.slot_off, tk, ts, tc, e, p)
        idx = np.concatenate([np.arange(s.slot_off[n], s.slot_off[n] + tc[n]) for n in range(s.n_nodes)]).astype(int)
        ora.add_batch(np.repeat(np.arange(s.n_nodes), tc), tk[idx], ts[idx], e, p)
        sizes.append(model.sizes())
        if on_add:
            on_add(a, model, ora)
    return model, ora, sizes


def by_node_key(items):
    k, nd, e, p = items
    order = np.lexsort((k, nd))
    return k[order], nd[order], e[order], p[order]


def compare(s, a, model, ora):
    """Per node: exact where the boundary was never tied, else the sorted target-zone energies."""
    mk, mn, me, mp = by_node_key(model.items())
    ok, on, oe, op = ora.items()
    op = op.view(np.uint64)
    for n in range(s.n_nodes):
        if n in model.overflowed:  # Go's unlimited tracker has no capacity
            continue
        m, o = mn == n, on == n
        assert sorted(me[m, s.zone].tolist()) == sorted(oe[o, s.zone].tolist()), (s.name, a, n)
        if n not in model.boundary_tied:
            for x, y in ((mk[m], ok[o]), (me[m], oe[o]), (mp[m], op[o])):
                np.testing.assert_array_equal(x, y, err_msg=f"{s.name} add {a} node {n}")


@pytest.mark.parametrize("s", SCENARIOS, ids=[s.name for s in SCENARIOS])
def test_model_against_go_heap(s):
    """Every device scenario, after every add.  An untied scenario has no tied node at all, so it is
    Go's result exactly: IDs, every zone's energy, power."""
    model, _, _ = run_both(s, lambda a, m, o: compare(s, a, m, o))
    if not s.tied:
        assert model.boundary_tied <= model.overflowed


def test_random_tied_sequences():
    """300 sequences: max_size in {1, 2, 5, 64, 100}, 1 to 50 distinct energy values, 5 adds of 0 to
    199 candidates.  Every one keeps Go's target-zone energies; IDs differ in some."""
    rng = np.random.default_rng(2024)
    id_differs = 0
    for i in range(300):
        s = tracker_cases.Scenario(f"random-{i}", "pod", 2, 1, int(rng.choice([1, 2, 5, 64, 100])), tied=True,
                                   seed=i)
        values = np.arange(1, int(rng.integers(1, 51)) + 1)
        s.node(*[rng.choice(values, size=int(rng.integers(0, 200))) for _ in range(5)])
        s.finish()
        model, ora, _ = run_both(s, lambda a, m, o: compare(s, a, m, o))
        id_differs += not np.array_equal(by_node_key(model.items())[0], ora.items()[0])
    assert id_differs > 0  # the sweep does reach the divergence


def test_divergence_example():
    """max_size 2; three single-item adds: 101 (5 µJ), 102 (5 µJ), 103 (9 µJ).  Go's heap pops its
    root for 103, the OLDER of the tied minima, and keeps {102, 103}; the rule evicts the item it
    ranks last, the NEWER one, and keeps {101, 103}.  The three arrive in different intervals, so no
    map order reconciles the two; the energies {5, 9} agree."""
    s = tracker_cases.divergence()
    model, ora, _ = run_both(s)
    mk, _, me, _ = model.items()
    ok, _, oe, _ = ora.items()
    assert mk.tolist() == [103, 101]  # in set order: energy descending
    assert sorted(ok.tolist()) == [102, 103]
    assert sorted(me[:, 0].tolist()) == sorted(oe[:, 0].tolist()) == [5, 9]


def test_model_basics():
    """max_size 0 keeps nothing; ties keep tracked items first, then list order; frozen copies."""
    e = np.array([[7, 1], [7, 2], [9, 3], [7, 4]], dtype=np.uint64)
    p = np.arange(8, dtype=np.float64).reshape(4, 2)
    off, tk, ts = [0, 4], [11, 12, 13, 14], [0, 1, 2, 3]
    off_model = TrackerModel(1, 2, 0, 0)
    off_model.add(off, tk, ts, [4], e, p)
    assert off_model.items()[0].size == 0
    m = TrackerModel(1, 2, 0, 3)
    m.add(off, tk, ts, [2], e, p)  # 11, 12 at 7
    m.add(off, tk[2:], ts[2:], [2], e, p)  # 13 at 9 goes first; 14 at 7 is behind 11 and 12: cut
    k, nd, ee, pp = m.items()
    assert k.tolist() == [13, 11, 12] and nd.tolist() == [0, 0, 0] and 0 in m.boundary_tied
    np.testing.assert_array_equal(ee, e[[2, 0, 1]])
    np.testing.assert_array_equal(pp, p[[2, 0, 1]].view(np.uint64))
    e[:] = 0  # the model's copies are its own
    np.testing.assert_array_equal(m.items()[2][:, 0], [9, 7, 7])


def test_inputs_reach_their_cases():
    """A condition on the inputs of the device tests, not a tolerance: at least half of the nodes
    with candidates in every tied scenario are tied at the retention boundary (an item equal in
    energy to the last one kept was dropped or never admitted); the sets meant to pass 512 do, inside
    an add and before they are full; the bounded maximum fills; the overflow overflows one node."""
    by_name = {}
    for s in SCENARIOS:
        model, _, sizes = run_both(s)
        by_name[s.name] = (s, model, sizes)
        busy = [n for n in range(s.n_nodes) if s.count[:, n].sum() > 0]
        assert s.n_nodes % 4 != 0  # four nodes share a workgroup
        if s.tied:
            assert 2 * len(model.boundary_tied) >= len(busy), (s.name, sorted(model.boundary_tied), busy)
        if s.n_nodes >= 6:  # empty nodes at the start, in the middle and at the end
            assert busy[0] > 0 and busy[-1] < s.n_nodes - 1
            assert set(range(busy[0], busy[-1])) - set(busy) or len(busy) == 1, s.name
    for name in ("big-tied-pod", "big-untied-proc", "big-tied-vm", "big-untied-pod"):
        s, model, sizes = by_name[name]
        full = [n for n in range(s.n_nodes) if s.count[0, n] == 300]
        assert len(full) == 2
        for n in full:
            per_add = [int(x[n]) for x in sizes]
            assert per_add == [300, 600, 900, 1200, 1500, 1500]  # 512 is passed inside add 1, by its 4th chunk
            assert (KSET_LDS - 300) % 64 != 0
        slow = [n for n in range(s.n_nodes) if s.count[0, n] == 90][0]
        assert [int(x[slow]) for x in sizes] == [90, 180, 270, 360, 450, 540]
    s, model, sizes = by_name["max-bounded"]
    assert [int(x[0]) for x in sizes] == [4000, 8000, 8192]
    assert len(set(s.energy[:, s.zone].tolist())) == 50 and len(set(model.items()[2][:, s.zone].tolist())) >= 30
    s, model, sizes = by_name["overflow"]
    assert model.overflowed == {s.over_node} and sizes[-1].tolist() == [0, 100, 90, 0, 100]
    s, model, sizes = by_name["after-overflow"]
    assert not model.overflowed and sizes[-1].tolist() == [0, 70, 100, 1, 30]
    s, model, _ = by_name["small-ties-proc"]
    k, nd, e, _ = model.items()
    assert k[nd == s.zero_node].tolist() == [tracker_cases.default_key(int(s.slot_off[s.zero_node]) + i)
                                             for i in range(5)]  # the first five listed, never evicted
    assert k[nd == s.pattern_node].tolist() == [201, 202, 203, 103, 101]
    assert k[nd == s.again_full].tolist() == [307, 306, 305, 304, 303]
    assert e[nd == s.again_full, s.zone].tolist() == [70, 60, 50, 40, 30]  # the first copies' energies
    assert k[nd == s.again_open].tolist() == [402, 404, 403, 401]
