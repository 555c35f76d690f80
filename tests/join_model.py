"""The table rules of the slot join, restated in plain Python (test-only).

THIS FILE MIRRORS kepler_amd/csrc/kacc_join.hip — node_buckets(), bucket(), the
h1 / h2 lambdas of join_small (kJCkFast) and step 6's ck_direct and kick loop —
AND MUST CHANGE WITH IT.  Nothing here is derived from running the kernel: each
rule is the source restated, so that a table read back from the device
(kacc_debug_slotmap_node) can be checked bucket by bucket.

A table is a pair of Python lists (keys, slots) of H entries; empty and
tombstone keys are the widened KACC_KEY_EMPTY / KACC_KEY_TOMB.

Formats (check_table's fmt):
  "cuckoo"    the production PID table of a small node: a key lives in one of
              the 4-bucket groups g1(k) / g2(k); terminated keys are emptied,
              there are no tombstones.
  "linear32"  PID table of a big node: linear probing from the Fibonacci home
              bucket, tombstones, rebuild when live + tombstones > 3/4 H.
  "linear64"  the same for the 64-bit IDs (the home bucket folds the high word in).
"""

EMPTY = 0xFFFFFFFFFFFFFFFF  # KACC_KEY_EMPTY
TOMB = 0xFFFFFFFFFFFFFFFE   # KACC_KEY_TOMB
M32 = 0xFFFFFFFF
MAX_KICKS = 512             # kCkMaxKicks

FORMATS = ("cuckoo", "linear32", "linear64")


class Homeless(Exception):
    """The kick loop ran out: `key` (with slot `rel`) fell out of the table.  The table is
    left as the kernel leaves it (the key given to place() is in; an older one is not)."""

    def __init__(self, key, rel):
        super().__init__(f"key {key} (slot {rel}) is homeless after {MAX_KICKS} kicks")
        self.key, self.rel = key, rel


def node_buckets(S):
    """Buckets of a node with S slots: a power of two >= 1.5 S and >= 64."""
    h = 64
    while h * 2 < 3 * S:
        h <<= 1
    return h


def _log2(x):
    assert x > 0 and x & (x - 1) == 0, x
    return x.bit_length() - 1


def groups(k, H):
    """(g1, g2) of PID k in a cuckoo table of H buckets (CG = H / 4 groups)."""
    csh = 32 - _log2(H // 4)
    g1 = ((k * 0x9E3779B1) & M32) >> csh
    g = (((k ^ (k >> 16)) * 0x85EBCA6B) & M32) >> csh
    return g1, (g if g != g1 else g1 ^ 1)


def home(k, H, wide):
    """Home bucket of the linear-probing tables (wide: a 64-bit ID, high word folded in)."""
    x = k & M32
    if wide:
        x ^= (k >> 32) & M32
    return ((x * 0x9E3779B1) & M32) >> (32 - _log2(H))


def new_table(H):
    return [EMPTY] * H, [0] * H


def _empties(keys, g):
    return [e for e in range(4) if keys[4 * g + e] == EMPTY]


def both_full(table, key):
    keys, _ = table
    g1, g2 = groups(key, len(keys))
    return not _empties(keys, g1) and not _empties(keys, g2)


def place(table, key, rel):
    """Place one new PID alone (no other insert in flight), as step 6 does: the lowest empty
    bucket of the emptier of its two groups, ties to the first group; both full: the kick
    loop.  Returns the chain length (evictions); 0 for a direct placement."""
    keys, slots = table
    H = len(keys)
    g1, g2 = groups(key, H)
    assert key not in keys[4 * g1:4 * g1 + 4] and key not in keys[4 * g2:4 * g2 + 4], f"{key} given twice"
    ea, eb = _empties(keys, g1), _empties(keys, g2)
    if ea or eb:  # ck_direct
        b = 4 * g1 + ea[0] if len(ea) >= len(eb) else 4 * g2 + eb[0]
        keys[b], slots[b] = key, rel
        return 0
    k = key
    for kick in range(MAX_KICKS):  # lane 0's loop
        ga, gb = groups(k, H)
        ea, eb = _empties(keys, ga), _empties(keys, gb)
        if ea or eb:  # here the FIRST group wins whenever it has room
            b = 4 * ga + ea[0] if ea else 4 * gb + eb[0]
            keys[b], slots[b] = k, rel
            return kick
        b = 4 * (gb if kick & 1 else ga) + ((kick >> 1) & 3)
        (keys[b], slots[b]), (k, rel) = (k, rel), (keys[b], slots[b])
    raise Homeless(k, rel)


def remove(table, key, fmt):
    """Terminate `key`: its bucket is emptied (cuckoo) or becomes a tombstone (linear)."""
    keys, _ = table
    b = keys.index(key)
    keys[b] = EMPTY if fmt == "cuckoo" else TOMB
    return b


def place_linear(table, key, rel, wide):
    """Linear probing: the first empty or tombstone bucket from the key's home bucket."""
    keys, slots = table
    H = len(keys)
    b = home(key, H, wide)
    for _ in range(H):
        if keys[b] in (EMPTY, TOMB):
            keys[b], slots[b] = key, rel
            return b
        b = (b + 1) & (H - 1)
    raise AssertionError("table full")


def check_table(dump, live, fmt):
    """dump = (keys, slots) of one node as read from the device; live = the expected
    {key: node-relative slot}.  Raises AssertionError naming the first broken rule."""
    assert fmt in FORMATS, fmt
    keys, slots = [int(k) for k in dump[0]], [int(s) for s in dump[1]]
    H = len(keys)
    assert H >= 64 and H & (H - 1) == 0 and len(slots) == H, f"bad bucket count {H}"
    seen = {}
    tombs = 0
    for b, k in enumerate(keys):
        if k == EMPTY:
            continue
        if k == TOMB:
            tombs += 1
            continue
        assert k in live, f"bucket {b}: key {k} is not live"
        assert k not in seen, f"key {k} in buckets {seen[k]} and {b}"
        seen[k] = b
        assert slots[b] == live[k], f"bucket {b}: key {k} has slot {slots[b]}, expected {live[k]}"
        if fmt == "cuckoo":
            assert b // 4 in groups(k, H), f"bucket {b}: key {k} is outside its groups {groups(k, H)}"
        else:
            p = home(k, H, fmt == "linear64")
            while p != b:  # a lookup stops at the first empty bucket
                assert keys[p] != EMPTY, f"key {k} in bucket {b} is cut off from its home by empty bucket {p}"
                p = (p + 1) & (H - 1)
    missing = [k for k in live if k not in seen]
    assert not missing, f"{len(missing)} live keys are not in the table, e.g. {missing[:4]}"
    if fmt == "cuckoo":
        assert tombs == 0, f"{tombs} tombstones in a cuckoo table"
    else:
        assert 4 * (len(seen) + tombs) <= 3 * H, f"live {len(seen)} + tombstones {tombs} > 3/4 of {H} buckets"


def tombstones(dump):
    return sum(1 for k in dump[0] if int(k) == TOMB)
