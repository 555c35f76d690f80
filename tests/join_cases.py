"""Fixed PID lists for the smallest cuckoo table (one node of 42 slots: 64 buckets, 16 groups),
found ahead of time with tests/join_model.py; tests/test_join_model.py asserts what each list
claims, tests/test_gpu_join_table.py feeds them to the device one new key per call.

Every PID is <= 2^22 (pid_max)."""

SLOTS = 42    # -> 64 buckets, 16 groups of 4
BUCKETS = 64

# groups of the single-kick case
A, B, B2, D = 4, 9, 13, 12

# nine PIDs whose two groups are B and B2 (in either order): eight fill both groups, whatever
# the order; the ninth has nowhere to go and no kick can free a bucket (every key of B and B2
# can only move between the two)
CONFINED9 = [3, 145, 166, 187, 414, 577, 598, 846, 1257]
CONFINED8 = CONFINED9[:8]
D_B = [286, 697, 3148]          # groups {D, B}: B is full, so they take three buckets of D
A_D = [227, 638, 1481, 2324]    # g1 = A, g2 = D: A is emptier (tie at the fourth: first group)
KICKER = 70                     # g1 = A, g2 = B: both full -> evicts A's bucket 0 into D
# one new key per call in this order: the last key is placed by exactly one kick
SINGLE_KICK = CONFINED8 + D_B + A_D + [KICKER]

# 42 PIDs (a full node), one per call: the last one finds both groups full and is placed by a
# chain of LONG_CHAIN_KICKS kicks
LONG_CHAIN = [
    204905, 685133, 1419836, 826921, 2062939, 527217, 2216458, 72736, 3773528, 227772, 2245543,
    3552234, 803557, 974013, 2632443, 2709159, 1180302, 570877, 3378330, 2244424, 1029964, 3580469,
    1890024, 3737682, 2106755, 2196079, 580721, 421594, 857591, 108082, 2118115, 2262762, 1095242,
    1433799, 28055, 2045912, 3227169, 139242, 2002934, 1379091, 386082, 1694527,
]
LONG_CHAIN_KICKS = 10
