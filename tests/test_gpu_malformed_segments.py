"""Malformed segment ends (ctr_proc_end / vm_proc_end / pod_ctr_end) through every node kernel —
MI355X only.

The header promises that "the kernel additionally clamps every index so a bad batch cannot
fault the GPU": a segment with beg < lo, end < beg or end > hi raises the offsets bit of
KACC_ERANGE and is clamped to beg = max(min(beg, hi), lo), end = max(min(end, hi), beg).
The rule is written in interval_kernel, small_kernel, intervals_carry_kernel and
chunk_kernel (+ pod_kernel); these tests feed each of them the same bad batches.

An end past the node's range is equivalent to the well-formed batch with that end at the
range's end, so the oracle decides.  end < beg / beg < p0 has no well-formed equivalent: the
kernels must agree with each other bit for bit and keep the damage inside the node.
"""

import re

import numpy as np
import pytest
import torch

from kepler_amd import accel, fleet
from kepler_amd.torch_batch import current_stream_handle, interval_from_tensors, to_device

pytestmark = pytest.mark.gpu

ERR_OFFSETS = 2  # "2=offsets" of kacc_sync's message: the second bit of the device error word
N_INTERVALS = 3
BAD = 1  # the interval (0-based) whose array is edited: totals before and after it matter


@pytest.fixture(scope="module", autouse=True)
def gpu_ready():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    accel.load()  # raises if the HIP library is missing: no fallback
    torch.cuda.set_stream(torch.cuda.Stream())


def assert_table_equal(got, want, msg):
    """Bit-exact, any NaN equal to any NaN (as smoke(): NaN bits are not an observable)."""
    if want.dtype.kind == "f":
        bad = (got.view(np.uint64) != want.view(np.uint64)) & ~(np.isnan(got) & np.isnan(want))
        assert not bad.any(), f"{msg}: {int(bad.sum())} differ, first at {int(np.flatnonzero(bad)[0])}"
    else:
        np.testing.assert_array_equal(got, want, err_msg=msg)


def error_bits(exc) -> int:
    assert exc.code == accel.KACC_ERANGE, str(exc)
    m = re.search(r"bits 0x([0-9a-f]+)", str(exc))
    assert m, str(exc)
    return int(m.group(1), 16)


def node_rows(layout, name, n):
    """Rows of table `name` that belong to node n (slots are consecutive per node here)."""
    kind = name.split("_")[0]
    off = dict(node=np.arange(layout.n_nodes + 1), proc=layout.proc_off, ctr=layout.ctr_off, vm=layout.vm_off,
               pod=layout.pod_off)[kind]
    return slice(int(off[n]), int(off[n + 1]))


def per_row(layout, name, table):
    kind = name.split("_")[0]
    rows = layout.n_nodes if kind == "node" else layout.capacities()[f"{kind}_slots"]
    return table.reshape(rows, -1)


def edits(layout, n):
    """The three bad arrays for node n: name -> (array, index, bad value, equivalent good value)."""
    p0, p1 = int(layout.proc_off[n]), int(layout.proc_off[n + 1])
    c0, c1 = int(layout.ctr_off[n]), int(layout.ctr_off[n + 1])
    v0, v1 = int(layout.vm_off[n]), int(layout.vm_off[n + 1])
    q1 = int(layout.pod_off[n + 1])
    assert c1 - c0 >= 3 and v1 > v0 and q1 > int(layout.pod_off[n])
    # the last segment in listing order is the last VM; rows past its end are free processes
    assert int(layout.vm_proc_end[v1 - 1]) < p1, "no free process behind the last VM: case (a) shows nothing"
    assert int(layout.pod_ctr_end[q1 - 1]) < c1, "no container outside the pods: case (b) shows nothing"
    mid = (c0 + c1) // 2
    assert c0 < mid < c1 - 1 and int(layout.ctr_proc_end[mid - 1]) > p0  # end < beg there, beg < p0 (or = p0) after
    return {
        "proc_end_past_p1": ("vm_proc_end", v1 - 1, p1 + 5, p1),
        "pod_end_past_c1": ("pod_ctr_end", q1 - 1, c1 + 3, c1),
        "end_below_beg": ("ctr_proc_end", mid, 0, None),
    }


def make_batches(layout, seed, edit):
    """Three intervals; interval BAD with one array edited on a copy -> (bad, good or None)."""
    sim = fleet.FleetSim(layout, seed=seed, churn=0.05)
    ivs = [sim.next_interval() for _ in range(N_INTERVALS)]
    name, i, bad_value, good_value = edit
    bad = [dict(a) for a in ivs]
    bad[BAD][name] = ivs[BAD][name].copy()
    bad[BAD][name][i] = bad_value
    good = None
    if good_value is not None:
        good = [dict(a) for a in ivs]
        good[BAD][name] = ivs[BAD][name].copy()
        good[BAD][name][i] = good_value
    return ivs, bad, good


def run_oracle(layout, ivs):
    from oracle.oracle import Oracle

    ora = Oracle(layout.zones, **layout.capacities())
    for a in ivs:
        ora.interval(a, layout.sizes())
    return ora.state


def assert_edit_shows(layout, ivs, want):
    """The equivalent well-formed batch must differ from the unedited one, or the case shows nothing."""
    plain = run_oracle(layout, ivs)
    assert any(not np.array_equal(plain[name], want[name], equal_nan=True) for name, _ in accel.TABLES)


def run_path(layout, ivs, path):
    """The three intervals through one kernel; returns (tables, error bits at sync)."""
    fast = layout.fast_flag()
    acc = accel.Accel(layout.zones, **layout.capacities())
    s = current_stream_handle()
    dev = [to_device(a) for a in ivs]
    if path == "carry_kernel":
        assert fast & accel.KACC_F_FAST_NODES and layout.zones <= 2
        flags = accel.KACC_F_FAST_NODES | accel.KACC_F_NODE_SLOT_RANGES
        acc.run_intervals([interval_from_tensors(t, layout.sizes(), flags) for t in dev], s)
    else:
        flags = dict(interval_kernel=fast & ~accel.KACC_F_SMALL_NODES, small_kernel=fast, chunk_kernel=fast)[path]
        assert bool(flags & accel.KACC_F_SMALL_NODES) == (path == "small_kernel")
        assert (flags == 0) == (path == "chunk_kernel")
        for t in dev:
            acc.run_interval(interval_from_tensors(t, layout.sizes(), flags), s)
    bits = 0
    try:
        acc.sync(s)
    except accel.AccelError as e:
        bits = error_bits(e)
    # host validation rejects the same batch before it reaches the GPU
    assert acc.validate_host(accel.make_interval(ivs[BAD], layout.sizes())) == accel.KACC_EINVAL
    tables = {name: acc.download(name) for name, _ in accel.TABLES}
    acc.close()
    return tables, bits


SMALL_PATHS = ["interval_kernel", "small_kernel", "carry_kernel"]


@pytest.fixture(scope="module")
def small_fleet():
    layout = fleet.make_layout(3, [70, 130, 40], 2, seed=43, vm_frac=0.05)
    assert np.all(np.diff(layout.ctr_off.astype(np.int64)) > 0) and np.all(np.diff(layout.vm_off.astype(np.int64)) > 0)
    assert np.all(np.diff(layout.pod_off.astype(np.int64)) > 0)
    assert layout.fast_flag() & accel.KACC_F_SMALL_NODES
    return layout


@pytest.fixture(scope="module")
def small_wellformed(small_fleet):
    ivs, _, _ = make_batches(small_fleet, 43, edits(small_fleet, 1)["end_below_beg"])
    return run_oracle(small_fleet, ivs)


@pytest.mark.parametrize("path", SMALL_PATHS)
@pytest.mark.parametrize("case", ["proc_end_past_p1", "pod_end_past_c1"])
def test_end_past_the_node_is_clamped_and_reported(small_fleet, case, path):
    """(a) the last VM of node 1 ends at p1 + 5, (b) the last pod of node 1 ends at c1 + 3:
    KACC_ERANGE with the offsets bit, and every table as the oracle's for the end at p1 / c1."""
    ivs, bad, good = make_batches(small_fleet, 43, edits(small_fleet, 1)[case])
    want = run_oracle(small_fleet, good)
    assert_edit_shows(small_fleet, ivs, want)
    got, bits = run_path(small_fleet, bad, path)
    assert bits & ERR_OFFSETS, hex(bits)
    for name, _ in accel.TABLES:
        assert_table_equal(got[name], want[name], f"{path} {case} {name}")


def test_end_below_begin_same_in_every_kernel(small_fleet, small_wellformed):
    """(c) a middle container of node 1 has ctr_proc_end = 0 (end < beg for it, beg < p0 for the
    next one): the three kernels give bit-identical tables, each reports the offsets bit, and
    nodes 0 and 2 are the oracle's well-formed run."""
    _, bad, _ = make_batches(small_fleet, 43, edits(small_fleet, 1)["end_below_beg"])
    results = {}
    for path in SMALL_PATHS:
        results[path], bits = run_path(small_fleet, bad, path)
        assert bits & ERR_OFFSETS, f"{path}: {hex(bits)}"
    ref = results["interval_kernel"]
    for path in SMALL_PATHS[1:]:
        for name, _ in accel.TABLES:
            assert_table_equal(results[path][name], ref[name], f"{path} vs interval_kernel {name}")
    for name, _ in accel.TABLES:
        g, w = per_row(small_fleet, name, ref[name]), per_row(small_fleet, name, small_wellformed[name])
        for n in (0, 2):
            r = node_rows(small_fleet, name, n)
            assert_table_equal(g[r].reshape(-1), w[r].reshape(-1), f"node {n} {name}")


@pytest.fixture(scope="module")
def big_fleet():
    layout = fleet.make_layout(2, [3000, 70], 4, seed=43, vm_frac=0.05)
    assert layout.fast_flag() == 0  # node 0 takes chunk_kernel + pod_kernel
    return layout


@pytest.mark.parametrize("case", ["proc_end_past_p1", "pod_end_past_c1"])
def test_big_node_end_past_the_node(big_fleet, case):
    """(d) the edits (a) and (b) on a 3000-process node (chunk_kernel + pod_kernel)."""
    ivs, bad, good = make_batches(big_fleet, 43, edits(big_fleet, 0)[case])
    want = run_oracle(big_fleet, good)
    assert_edit_shows(big_fleet, ivs, want)
    got, bits = run_path(big_fleet, bad, "chunk_kernel")
    assert bits & ERR_OFFSETS, hex(bits)
    for name, _ in accel.TABLES:
        assert_table_equal(got[name], want[name], f"chunk_kernel {case} {name}")


def test_big_node_end_below_begin(big_fleet):
    """(d) the edit (c) on the big node: the offsets bit, the small node untouched, and a clean
    interval after it runs without error."""
    layout = big_fleet
    ivs, bad, _ = make_batches(layout, 43, edits(layout, 0)["end_below_beg"])
    want = run_oracle(layout, ivs[:BAD + 1])
    acc = accel.Accel(layout.zones, **layout.capacities())
    s = current_stream_handle()
    dev = [to_device(a) for a in bad]
    descs = [interval_from_tensors(t, layout.sizes(), 0) for t in dev]
    acc.run_interval(descs[0], s)
    acc.sync(s)
    acc.run_interval(descs[BAD], s)
    with pytest.raises(accel.AccelError) as ei:
        acc.sync(s)
    assert error_bits(ei.value) & ERR_OFFSETS
    assert acc.validate_host(accel.make_interval(bad[BAD], layout.sizes())) == accel.KACC_EINVAL
    for name, _ in accel.TABLES:
        g, w = per_row(layout, name, acc.download(name)), per_row(layout, name, want[name])
        r = node_rows(layout, name, 1)
        assert_table_equal(g[r].reshape(-1), w[r].reshape(-1), f"node 1 {name}")
    acc.run_interval(descs[2], s)
    acc.sync(s)  # a clean interval: no error left over, none raised
    acc.close()
