"""The host arithmetic of the row queries (kepler_amd/csrc/kacc_plan.hpp), without a GPU.

tests/c/rows_plan.cpp includes only that header and is built by the host compiler alone, once
plainly and once with the address and undefined-behaviour sanitizers; both runs answer the same
requests.  The LDS plans are held against tests/plan_ref.py (the restatements the GPU tests use
to show that their shapes reach every regime) at every capacity boundary, which the test derives
from the constants, and over a sweep of group counts.  The scratch layout is held to its three
rules - every array at a multiple of its element size, no two arrays overlapping, the total the
last array's end - for the units' own declarations and for mixed ones, and to the byte counts the
entry points allocated and zeroed before the layout computed them.
"""

import os
import subprocess

import pytest

import plan_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "rows_plan.cpp")
CUS = 256
PER_CU = {"group": {"small": 3, "big": 2, "over": 2}, "hist": {"small": 3, "big": 1, "over": 2},
          "window": {"small": 3, "big": 2, "over": 8}}
ZONES = (4, 5)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def program(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rows_plan") / request.param)
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, SRC, "-o", exe], check=True)

    def ask(lines):
        r = subprocess.run([exe], input="".join(f"{x}\n" for x in lines), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and not r.stderr, r.stderr
        out = r.stdout.splitlines()
        assert len(out) == len(lines)
        return out

    return ask


# ---- the LDS plans ----------------------------------------------------------------------------


def last_that_fits(fits):
    """The largest group count that still `fits`; (g, g + 1) straddles the capacity."""
    g = 1
    while fits(g + 1):
        g += 1
    return g


def group_pairs(z):
    w = 1 + 2 * z
    per_pass = P.GROUP_PASS_WORDS // w
    return {"small": last_that_fits(lambda g: ((g * w) | 1) <= P.GROUP_SMALL_WORDS),
            "big": last_that_fits(lambda g: g * w <= P.GROUP_BIG_WORDS),  # one copy | two passes
            "two": 2 * per_pass}                                          # two | three passes


def window_pairs(z):
    w = 1 + z
    return {"small": last_that_fits(lambda g: ((g * w) | 1) <= P.WINDOW_SMALL_WORDS),
            "big": last_that_fits(lambda g: g * w <= P.WINDOW_BIG_WORDS)}


def hist_pairs(n_bounds):
    c = n_bounds + 3
    per = lambda g: ((g * c) | 1) + 2 * (g | 1)  # noqa: E731
    return {"copies": last_that_fits(lambda g: 2 * per(g) <= P.HIST_SMALL_WORDS),
            "small": last_that_fits(lambda g: per(g) <= P.HIST_SMALL_WORDS),
            "big": last_that_fits(lambda g: g * (c + 2) <= P.HIST_BIG_WORDS),
            "two": 2 * (P.HIST_PASS_WORDS // (c + 2))}


def expected_bins(unit, g, p, tiles, pass_tiles):
    """The answer line of rows_plan.cpp from the restatements."""
    if unit == "group":
        copies, passes, where = P.group_regime(g, p)
        bins = P.GROUP_PASS_WORDS // (1 + 2 * p) if where == "pass" else g
    elif unit == "hist":
        copies, passes, where = P.hist_regime(g, p)
        bins = P.HIST_PASS_WORDS // (p + 5) if where == "pass" else g
    else:
        (copies, where), passes, bins = P.window_regime(g, p), 1, g
    regime = "over" if where in ("pass", "global") else where
    wgs = CUS * PER_CU[unit][regime]
    splits = max(1, min(pass_tiles, wgs // passes) if passes > 1 else min(tiles, wgs))
    return f"{regime} {copies} {bins} {passes} {wgs} {splits}"


def test_the_pairs_are_the_capacities():
    # the pairs tests/test_gpu_hist.py lists in SHAPES, here from the constants
    assert hist_pairs(15) == {"copies": 204, "small": 409, "big": 1004, "two": 1920}
    for z in ZONES:
        g = group_pairs(z)
        assert P.group_regime(g["small"], z)[2] == "small" and P.group_regime(g["small"] + 1, z) == (1, 1, "big")
        assert P.group_regime(g["big"], z) == (1, 1, "big") and P.group_regime(g["big"] + 1, z) == (1, 2, "pass")
        assert P.group_regime(g["two"], z) == (1, 2, "pass") and P.group_regime(g["two"] + 1, z) == (1, 3, "pass")
        w = window_pairs(z)
        assert P.window_regime(w["small"], z)[1] == "small" and P.window_regime(w["small"] + 1, z) == (1, "big")
        assert P.window_regime(w["big"], z) == (1, "big") and P.window_regime(w["big"] + 1, z) == (1, "global")
    # the comments of kacc_group.hip and kacc_window.hip
    assert group_pairs(4)["big"] == 1109 and group_pairs(4)["two"] == 2 * 1080 and window_pairs(4)["big"] == 1996


def test_bins_plans_match_the_restatements(program):
    asks = []
    for z in ZONES:
        for unit, pairs in (("group", group_pairs(z)), ("window", window_pairs(z))):
            for g in sorted({1, 2, 7, 63, 1000, 65536} | {b + d for b in pairs.values() for d in (0, 1)}):
                asks.append((unit, g, z))
        asks += [(unit, g, z) for unit in ("group", "window") for g in range(1, 2600, 3)]
    for n_bounds in (1, 3, 7, 15, 64):
        groups = {1, 2, 63, 1000, 1025, 16131} | {b + d for b in hist_pairs(n_bounds).values() for d in (0, 1)}
        asks += [("hist", g, n_bounds) for g in sorted(groups) if g * (n_bounds + 1) <= 1 << 20]
    asks += [("hist", g, 15) for g in (204, 205, 409, 410, 1004, 1005, 1920, 1921, 65536)]
    asks += [("hist", g, 15) for g in range(1, 2600, 3)]
    lines, want = [], []
    for unit, g, p in asks:
        # few tiles, as many as resident workgroups, more; a pass's tiles are twice as long
        for tiles in (0, 1, 500, 100000):
            pass_tiles = (tiles + 1) // 2
            lines.append(f"{unit} {g} {p} {tiles}" + ("" if unit == "window" else f" {pass_tiles}"))
            want.append(f"{lines[-1]} {expected_bins(unit, g, p, tiles, pass_tiles)}")
    assert program(lines) == want


def test_digit_plans_match_the_restatements(program):
    # (n_groups, n_phi) of tests/test_gpu_quant.py's boundary pairs, 64 queries among them
    quant = [(1, 1), (1, 8), (7, 1), (3, 5), (31, 1), (32, 1), (4, 8), (64, 1), (8, 8), (65, 1), (13, 5), (1000, 3),
             (8192, 8), (65536, 1)]
    counters = sorted({g * p for g, p in quant} | set(range(1, 70)) | {1000, 1024, 65536})
    got = program([f"digit {n}" for n in counters])
    assert got == [f"digit {n} {P.gtop_regime(n)[0]}" for n in counters]
    for g, p in quant:
        assert P.quant_regime(g, p) == P.gtop_regime(g * p)
        assert got[counters.index(g * p)] == f"digit {g * p} {P.quant_regime(g, p)[0]}"


# ---- the scratch layout -----------------------------------------------------------------------


def round8(n):
    return (n + 7) & ~7


def unit_layouts():
    """(name, [(elem, count, zeroed)], the parent's bytes, the parent's zeroed bytes or None)."""
    out = []
    for g, n_phi, n_rows, n_nodes in ((1, 1, 0, 0), (2, 1, 0, 0), (3, 5, 1, 1), (7, 1, 4097, 33), (64, 1, 100000, 1000)):
        q = g * n_phi
        zeroed = round8(4 * q * 256 + 16 * q + 12 * q + 4 * g)
        out.append((f"quant{g}x{n_phi}", [(4, q * 256, 1), (8, q, 1), (8, q, 1), (4, q, 1), (4, q, 1), (4, q, 1), (4, g, 1),
                                         (8, n_rows, 0), (4, n_rows, 0), (4, n_nodes, 0)],
                    zeroed + 12 * n_rows + 4 * n_nodes, zeroed))
    for g, k, n_rows, n_nodes in ((1, 1, 0, 0), (2, 3, 5, 2), (7, 10, 4097, 33), (1000, 3, 100000, 1000)):
        zeroed = round8(4 * g * 256 + 8 * g + 5 * 4 * g + 4)
        out.append((f"gtop{g}x{k}", [(4, g * 256, 1), (8, g, 1)] + [(4, g, 1)] * 5 + [(4, 1, 1), (8, n_rows, 0), (8, g * k, 0),
                                                                                   (4, n_rows, 0), (4, g * k, 0), (4, n_nodes, 0)],
                    zeroed + 12 * n_rows + 12 * g * k + 4 * n_nodes, zeroed))
    for g, z, n_rows, n_nodes in ((1, 4, 0, 0), (3, 5, 0, 7), (1110, 4, 4097, 33)):
        acc = g * (1 + 2 * z)
        out.append((f"group{g}z{z}", [(8, acc, 1), (4, n_nodes, 0), (4, n_rows, 0), (4, n_rows, 0)],
                    8 * acc + 4 * n_nodes + 8 * n_rows, 8 * acc))
        out.append((f"window{g}z{z}", [(8, g * (1 + z), 1), (4, n_nodes, 0)], 8 * g * (1 + z) + 4 * n_nodes, 8 * g * (1 + z)))
    for g, n_bounds, n_rows, n_nodes in ((1, 1, 0, 0), (1005, 15, 4097, 33)):
        acc = g * (n_bounds + 4)
        out.append((f"hist{g}x{n_bounds}", [(8, acc, 1), (8, n_rows, 0), (4, n_rows, 0), (4, n_nodes, 0)],
                    8 * acc + 12 * n_rows + 4 * n_nodes, 8 * acc))
    for tiles, scan_tiles, n_nodes in ((0, 1, 1), (3, 1, 33)):  # the selection: mask, counts, offsets, the scan's sums
        out.append((f"select{tiles}", [(8, tiles * 32, 0), (8, tiles + 1, 0), (8, tiles + 1, 0), (8, scan_tiles, 0), (4, n_nodes, 0)],
                    8 * (tiles * 32 + 2 * (tiles + 1) + scan_tiles) + 4 * n_nodes, None))
    for ents, lists in ((0, 0), (10, 2), (4096, 5)):  # the fleet's candidate lists: 8-byte keys, rows, nodes, counts
        out.append((f"fleet{ents}", [(8, ents, 0), (4, ents, 0), (4, ents, 0), (4, lists, 0)], 16 * ents + 4 * lists, None))
    out.append(("step", [(4, 33, 0)], 4 * 33, None))
    out.append(("none", [], 0, None))
    # no unit's: every element size, empty arrays, a zeroed prefix that ends off an 8-byte word
    out.append(("mixed", [(1, 3, 1), (8, 2, 1), (2, 5, 1), (4, 0, 0), (16, 3, 0), (1, 1, 0), (2, 1, 0), (8, 0, 0), (4, 3, 0)], None, None))
    out.append(("tail", [(8, 1, 1), (4, 1, 1)], None, None))
    out.append(("bytes", [(1, 1, 1), (1, 1, 0)], None, None))
    return out


def test_layout_rules(program):
    layouts = unit_layouts()
    got = program(["layout " + " ".join(f"{e}:{n}:{z}" for e, n, z in decls) for _, decls, _, _ in layouts])
    for (name, decls, parent_bytes, parent_zeroed), line in zip(layouts, got):
        words = line.split()
        assert words[0] == "layout" and len(words) == 3 + len(decls), name
        total, zeroed, offs = int(words[1]), int(words[2]), [int(w) for w in words[3:]]
        spans = [(off, off + e * n) for off, (e, n, _) in zip(offs, decls)]
        for (off, _), (e, _, _) in zip(spans, decls):
            assert off % e == 0, name                       # a multiple of the element size
        for (_, end), (nxt, _) in zip(spans, spans[1:]):
            assert end <= nxt, name                         # in order: no two arrays overlap
        assert total == (spans[-1][1] if spans else 0), name  # the last offset plus the last size
        # the one memset covers the zeroed arrays, whole 8-byte words of them, inside the allocation
        z_end = max([end for (_, end), (_, _, z) in zip(spans, decls) if z], default=0)
        assert zeroed == min(round8(z_end), total), name
        if parent_bytes is not None:
            assert total == parent_bytes, name
        if parent_zeroed is not None:
            assert zeroed == min(parent_zeroed, total), name
            assert zeroed == parent_zeroed or not any(n for _, n, z in decls if not z), name  # only without a row, a node
