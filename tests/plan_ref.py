"""The LDS plans of the group queries, restated from kepler_amd/csrc/kacc_plan.hpp.

One restatement per unit: which regime the library picks for a shape, with how many copies of the
bins or counters and how many passes.  tests/test_rows_plan.py holds them against the C++ on the
CPU; the GPU tests of the units use them to show that their shapes reach every regime.
"""

MAX_COPIES = 64

# kacc_hist.hip's LDS capacities in u32 words, restated; a group takes n_bounds + 5 of them
HIST_SMALL_WORDS, HIST_BIG_WORDS, HIST_PASS_WORDS = 8192, 20096, 19200
# kacc_group.hip's in u64 words; a group takes 1 + 2Z of them
GROUP_SMALL_WORDS, GROUP_BIG_WORDS, GROUP_PASS_WORDS = 4096, 9984, 9728
# the read of kacc_window.hip, in u64 words; a group takes 1 + Z of them, and there are no passes
WINDOW_SMALL_WORDS, WINDOW_BIG_WORDS = 4096, 9984
# kacc_quant.hip's and kacc_gtop.hip's: 256 u32 counters per query or group, 16384 words of LDS
DIGITS, LDS_WORDS = 256, 16384


def copies_that_fit(per_copy, words):
    copies = 1
    while copies < MAX_COPIES and 2 * copies * per_copy <= words:
        copies *= 2
    return copies


def hist_regime(n_groups, n_bounds):
    """(copies, passes) the library picks: copies > 1 = replicated counters in the small LDS size,
    (1, 1) = one copy (small or large), passes > 1 = the row-word passes."""
    c = n_bounds + 3
    per = ((n_groups * c) | 1) + 2 * (n_groups | 1)
    if per <= HIST_SMALL_WORDS:
        copies = 1
        while copies < MAX_COPIES and 2 * copies * per <= HIST_SMALL_WORDS:
            copies *= 2
        return copies, 1, "small"
    if n_groups * (c + 2) <= HIST_BIG_WORDS:
        return 1, 1, "big"
    per_pass = HIST_PASS_WORDS // (c + 2)
    return 1, -(-n_groups // per_pass), "pass"


def quant_regime(n_groups, n_phi):
    """(copies, where) the library picks: copies > 1 = replicated LDS counters, (1, "lds") = one
    copy, (0, "global") = global atomics."""
    words = n_groups * n_phi * DIGITS
    if words > LDS_WORDS:
        return 0, "global"
    copies = 1
    if 2 * (words | 1) <= LDS_WORDS:
        while copies < MAX_COPIES and 2 * copies * (words | 1) <= LDS_WORDS:
            copies *= 2
    return copies, "lds"


def gtop_regime(n_groups):
    """(copies, where) the library picks: copies > 1 = replicated LDS counters, (1, "lds") = one
    copy, (0, "global") = global atomics."""
    words = n_groups * DIGITS
    if words > LDS_WORDS:
        return 0, "global"
    copies = 1
    if 2 * (words | 1) <= LDS_WORDS:
        while copies < MAX_COPIES and 2 * copies * (words | 1) <= LDS_WORDS:
            copies *= 2
    return copies, "lds"


def group_regime(n_groups, zones):
    """kacc_group_sums: (copies, passes, where) for bins of 1 + 2Z u64 words a group."""
    w = 1 + 2 * zones
    stride = (n_groups * w) | 1
    if stride <= GROUP_SMALL_WORDS:
        return copies_that_fit(stride, GROUP_SMALL_WORDS), 1, "small"
    if n_groups * w <= GROUP_BIG_WORDS:
        return 1, 1, "big"
    return 1, -(-n_groups // (GROUP_PASS_WORDS // w)), "pass"


def window_regime(n_groups, zones):
    """kacc_window_read: (copies, where) for bins of 1 + Z u64 words a group; past the large LDS
    size the rows add into the accumulator itself."""
    w = 1 + zones
    stride = (n_groups * w) | 1
    if stride <= WINDOW_SMALL_WORDS:
        return copies_that_fit(stride, WINDOW_SMALL_WORDS), "small"
    return 1, "big" if n_groups * w <= WINDOW_BIG_WORDS else "global"
