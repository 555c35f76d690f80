"""tests/join_model.py on its own (CPU): check_table can fail, the fixed PID lists of
join_cases.py do what they claim, and the coverage claim behind test_gpu_join_table.py —
the shapes of test_gpu_join.py never reach the kick loop, 2,730 rows in 4,096 buckets do.
"""

import copy
import random

import numpy as np
import pytest

from kepler_amd import fleet
import join_cases as jc
import join_model as jm


def fill(keys, H):
    """One key per placement, slots in order; returns (table, chain lengths)."""
    t = jm.new_table(H)
    return t, [jm.place(t, k, i) for i, k in enumerate(keys)]


def test_node_buckets():
    assert [jm.node_buckets(s) for s in (0, 1, 42, 43, 2730, 2731, 3653, 131072)] == \
        [64, 64, 64, 128, 4096, 8192, 8192, 262144]


def test_groups_differ_and_stay_in_range():
    rng = random.Random(3)
    for H in (64, 1024, 4096):
        for k in [0, 1, 2, 1 << 22, 0xFFFFFFFD] + [rng.randrange(1 << 32) for _ in range(2000)]:
            g1, g2 = jm.groups(k, H)
            assert g1 != g2 and 0 <= g1 < H // 4 and 0 <= g2 < H // 4


# ---- check_table rejects every corruption of a good dump ---------------------------------


@pytest.fixture(scope="module")
def good_cuckoo():
    keys = jc.SINGLE_KICK
    t, _ = fill(keys, jc.BUCKETS)
    live = {k: i for i, k in enumerate(keys)}
    jm.check_table(t, live, "cuckoo")
    return t, live


@pytest.fixture(scope="module", params=["linear32", "linear64"])
def good_linear(request):
    """30 keys of 64 buckets with a chain that wraps past the end and one tombstone."""
    fmt, wide = request.param, request.param == "linear64"
    H, rng = 64, random.Random(5)
    keys = []
    while len(keys) < 30:
        k = rng.randrange(1, 1 << (60 if wide else 22))
        if k not in keys and (len(keys) >= 6 or jm.home(k, H, wide) >= H - 2):
            keys.append(k)
    t = jm.new_table(H)
    for i, k in enumerate(keys):
        jm.place_linear(t, k, i, wide)
    live = {k: i for i, k in enumerate(keys)}
    jm.remove(t, keys[0], fmt)  # a tombstone at the head of the wrapping chain
    del live[keys[0]]
    assert any(t[0][b] != jm.EMPTY for b in range(4)), "the chain wraps"
    jm.check_table(t, live, fmt)
    return t, live, fmt


def test_check_rejects_removed_key(good_cuckoo):
    t, live = copy.deepcopy(good_cuckoo)
    jm.remove(t, jc.KICKER, "cuckoo")
    with pytest.raises(AssertionError, match="not in the table"):
        jm.check_table(t, live, "cuckoo")


def test_check_rejects_key_in_third_group(good_cuckoo):
    t, live = copy.deepcopy(good_cuckoo)
    k = jc.KICKER
    b = jm.remove(t, k, "cuckoo")
    third = next(g for g in range(16) if g not in jm.groups(k, 64) and jm.EMPTY in t[0][4 * g:4 * g + 4])
    nb = 4 * third + t[0][4 * third:4 * third + 4].index(jm.EMPTY)
    t[0][nb], t[1][nb] = k, t[1][b]
    with pytest.raises(AssertionError, match="outside its groups"):
        jm.check_table(t, live, "cuckoo")


def test_check_rejects_swapped_slots(good_cuckoo):
    t, live = copy.deepcopy(good_cuckoo)
    b0, b1 = t[0].index(jc.KICKER), t[0].index(jc.A_D[0])
    t[1][b0], t[1][b1] = t[1][b1], t[1][b0]
    with pytest.raises(AssertionError, match="has slot"):
        jm.check_table(t, live, "cuckoo")


def test_check_rejects_duplicate_in_other_group():
    keys = jc.SINGLE_KICK[:-1]
    t, live = fill(keys, jc.BUCKETS)[0], {k: i for i, k in enumerate(keys)}
    jm.check_table(t, live, "cuckoo")
    k = jc.A_D[1]  # sits in A; D has an empty bucket left
    b = t[0].index(k)
    other = next(g for g in jm.groups(k, 64) if g != b // 4)
    nb = 4 * other + t[0][4 * other:4 * other + 4].index(jm.EMPTY)
    t[0][nb], t[1][nb] = k, t[1][b]
    with pytest.raises(AssertionError, match="in buckets"):
        jm.check_table(t, live, "cuckoo")


def test_check_rejects_dead_key_and_tombstone(good_cuckoo):
    t, live = copy.deepcopy(good_cuckoo)
    less = {k: s for k, s in live.items() if k != jc.KICKER}
    with pytest.raises(AssertionError, match="not live"):  # nothing else is live
        jm.check_table(t, less, "cuckoo")
    jm.remove(t, jc.KICKER, "linear32")
    with pytest.raises(AssertionError, match="tombstones in a cuckoo"):
        jm.check_table(t, less, "cuckoo")


def test_check_rejects_empty_in_probe_chain(good_linear):
    t, live, fmt = copy.deepcopy(good_linear)
    wide = fmt == "linear64"
    H = len(t[0])
    # a live key away from its home bucket: empty the first bucket of its path (the tombstone
    # at the head of the wrapping chain, or another key's bucket)
    k, b = next((k, b) for b, k in enumerate(t[0]) if k in live and jm.home(k, H, wide) != b)
    p = jm.home(k, H, wide)
    live = {kk: s for kk, s in live.items() if kk != t[0][p]}
    t[0][p] = jm.EMPTY
    with pytest.raises(AssertionError, match="cut off"):
        jm.check_table(t, live, fmt)


def test_check_rejects_crowded_linear_table(good_linear):
    t, live, fmt = copy.deepcopy(good_linear)
    for b in range(len(t[0])):
        if t[0][b] == jm.EMPTY and jm.tombstones(t) + len(live) < 49:  # 49 > 3/4 of 64
            t[0][b] = jm.TOMB
    with pytest.raises(AssertionError, match="3/4"):
        jm.check_table(t, live, fmt)


# ---- the fixed lists --------------------------------------------------------------------


def test_case_keys_are_pids():
    for lst in (jc.CONFINED9, jc.SINGLE_KICK, jc.LONG_CHAIN):
        assert len(set(lst)) == len(lst) and all(0 < k <= 1 << 22 for k in lst)
    assert len(jc.SINGLE_KICK) <= jc.SLOTS and len(jc.LONG_CHAIN) == jc.SLOTS
    assert jm.node_buckets(jc.SLOTS) == jc.BUCKETS


def test_confined_keys_share_one_pair_of_groups():
    for k in jc.CONFINED9:
        assert set(jm.groups(k, 64)) == {jc.B, jc.B2}
    for seed in range(5):  # eight fill both groups in any order; the ninth is homeless
        keys = jc.CONFINED9[:]
        random.Random(seed).shuffle(keys)
        t, chains = fill(keys[:8], 64)
        assert chains == [0] * 8
        assert all(k != jm.EMPTY for k in t[0][4 * jc.B:4 * jc.B + 4] + t[0][4 * jc.B2:4 * jc.B2 + 4])
        with pytest.raises(jm.Homeless) as ei:
            jm.place(t, keys[8], 8)
        # the key that falls out is an OLD one; the new one is in the table
        assert ei.value.key in keys[:8] and keys[8] in t[0]


def test_single_kick_list():
    for k in jc.D_B:
        assert set(jm.groups(k, 64)) == {jc.D, jc.B}
    for k in jc.A_D:
        assert jm.groups(k, 64) == (jc.A, jc.D)
    assert jm.groups(jc.KICKER, 64) == (jc.A, jc.B)
    t, chains = fill(jc.SINGLE_KICK[:-1], 64)
    assert chains == [0] * 15
    assert t[0][4 * jc.A:4 * jc.A + 4] == jc.A_D
    assert sum(k == jm.EMPTY for k in t[0][4 * jc.D:4 * jc.D + 4]) == 1
    assert jm.both_full(t, jc.KICKER)
    assert jm.place(t, jc.KICKER, 15) == 1
    assert t[0][4 * jc.A] == jc.KICKER and t[0][4 * jc.D + 3] == jc.A_D[0]  # A's bucket 0 went to D
    jm.check_table(t, {k: i for i, k in enumerate(jc.SINGLE_KICK)}, "cuckoo")


def test_long_chain_list():
    t, chains = fill(jc.LONG_CHAIN[:-1], 64)
    assert jm.both_full(t, jc.LONG_CHAIN[-1])
    n = jm.place(t, jc.LONG_CHAIN[-1], 41)
    assert n == jc.LONG_CHAIN_KICKS and n >= 5
    jm.check_table(t, {k: i for i, k in enumerate(jc.LONG_CHAIN)}, "cuckoo")


# ---- which shapes reach the kick loop ---------------------------------------------------


def deferred(rows, seed):
    """Keys of a fill of a 4,096-bucket table with the suite's PIDs (fleet.KeyedChurn, as
    test_gpu_join.py draws them) that find both groups full, placed one at a time."""
    sim = fleet.KeyedChurn(np.array([0, rows], dtype=np.uint32), seed=seed, churn=0.05, kind="proc")
    t = jm.new_table(4096)
    n = 0
    for i, k in enumerate(sim.next_keys().tolist()):
        n += jm.both_full(t, k)
        jm.place(t, k, i)
    return n


@pytest.mark.parametrize("seed", [7, 11, 12])  # 7 and 11: the seeds test_gpu_join.py uses
def test_coverage_claim(seed):
    """The largest small-table fill of test_gpu_join.py (2,184 rows) never defers a key; a full
    2,730-row node (test_gpu_join_table.py) does."""
    assert deferred(2184, seed) == 0
    assert deferred(2730, seed) >= 1
