#!/usr/bin/env python3
"""Value histograms of the running workloads at config 3 (10k nodes x 2k processes, Z = 4) on one
MI355X: kacc_group_hist with every output on, 15 decade bounds, for the process power of zone 0
with 1 group (group NULL), 8, 1000 and 65 536 random groups and 10 000 per-node groups, and for the
pod energy by namespace.

Yardsticks, measured in the same run on the same box and reported as ratios (the parent commit has
no counterpart, so nothing is gated on an absolute time): kacc_group_sums with the same ids and
every output (it moves strictly more bytes per row), and kacc_select_above at threshold 0 on the
same table and zone, with every output and as the sizing call (item_cap 0: the predicate pass
alone).

One HIP event pair around --calls back-to-back calls after --warmup calls; ms per call is the
window over the calls; the median of --reps windows.
Algorithmic bytes of a call, per row: with one pass the slot word (4), the group id (4; none with
group NULL) and the value (8: the ratio of a derived power, or the table's word of the zone); with
several passes 28 for the classify pass (slot word, id and value read, the 4-byte row word and the
8-byte sum word written), 4 per pass for the row words, and 12 in the owning pass (the row word
again and the sum word).  Writes one JSON object to --out and prints it.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_SPEC_GBPS = 8000.0
SMALL_WORDS, BIG_WORDS, PASS_WORDS = 8192, 20096, 19200  # kacc_hist.hip: kSmallWords, kBigWords, kPassWords
GROUP_SMALL, GROUP_BIG, GROUP_PASS = 4096, 9984, 9728    # kacc_group.hip's, in u64


def regime_of(n_groups, n_bounds):
    """(copies, passes) kacc_hist.hip runs with."""
    c = n_bounds + 3
    per = ((n_groups * c) | 1) + 2 * (n_groups | 1)
    if per <= SMALL_WORDS:
        copies = 1
        while copies < 64 and 2 * copies * per <= SMALL_WORDS:
            copies *= 2
        return copies, 1
    if n_groups * (c + 2) <= BIG_WORDS:
        return 1, 1
    bins = PASS_WORDS // (c + 2)
    return 1, (n_groups + bins - 1) // bins


def group_passes_of(n_groups, zones):
    w = 1 + 2 * zones
    if ((n_groups * w) | 1) <= GROUP_SMALL or n_groups * w <= GROUP_BIG:
        return 1
    bins = GROUP_PASS // w
    return (n_groups + bins - 1) // bins


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=0, help="nodes of the config 3 fleet (0: 10000)")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "hist", "bench.json"))
    args = ap.parse_args()

    import torch

    from kepler_amd import accel, fleet
    from kepler_amd.torch_batch import current_stream_handle, interval_from_tensors, to_device, top_rows_from_tensors

    torch.cuda.set_device(0)
    torch.cuda.set_stream(torch.cuda.Stream())
    s = current_stream_handle()
    L = fleet.config_layout(3, nodes=args.nodes or None)
    Z, N, P, Q = L.zones, L.n_nodes, L.n_procs, L.n_pods
    sim = fleet.FleetSim(L)
    acc = accel.Accel(Z, **L.capacities())
    sizes, flags = L.sizes(), L.fast_flag()
    t = a = None
    for _ in range(2):  # the second interval has powers
        a = sim.next_interval()
        t = to_device(a)
        acc.run_interval(interval_from_tensors(t, sizes, flags), s)
    acc.sync(s)

    def timed(call):
        for _ in range(args.warmup):
            call()
        acc.sync(s)
        ms = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                call()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / args.calls)
        acc.sync(s)
        return float(np.median(ms)), ms

    kinds = {"proc": (accel.KACC_KIND_PROC, P), "pod": (accel.KACC_KIND_POD, Q)}
    rows = {k: top_rows_from_tensors(t, kinds[k][0]) for k in kinds}
    rng = np.random.default_rng(1)
    i64 = lambda n: torch.empty(n, dtype=torch.int64, device="cuda")  # noqa: E731

    def hist_call(table, kind, d_group, n_groups, bounds):
        b1 = len(bounds) + 1
        out = (i64(n_groups * b1), i64(n_groups * b1), i64(n_groups), i64(n_groups), i64(n_groups))
        ptrs = [x.data_ptr() for x in out]

        def call():
            acc.group_hist(table, 0, rows[kind], d_group.data_ptr() if d_group is not None else 0, n_groups, bounds, 0,
                           *ptrs, s)
        return call, out

    def group_call(kind, d_group, n_groups):
        cnt = torch.empty(n_groups, dtype=torch.int32, device="cuda")
        drp = torch.empty(n_groups, dtype=torch.int32, device="cuda")
        e, fx = i64(n_groups * Z), i64(n_groups * Z)
        p = torch.empty(n_groups * Z, dtype=torch.float64, device="cuda")

        def call():
            acc.group_sums(kinds[kind][0], rows[kind], d_group.data_ptr(), n_groups, 0, cnt.data_ptr(), e.data_ptr(),
                           fx.data_ptr(), p.data_ptr(), drp.data_ptr(), s)
        return call, (cnt, e, fx, p, drp)

    select_keep = []

    def select_call(table, kind, item_cap):
        n = kinds[kind][1]
        out = (torch.zeros(N + 1, dtype=torch.int32, device="cuda"),
               *(torch.empty(max(item_cap, 1), dtype=torch.int32, device="cuda") for _ in range(3)),
               i64(max(item_cap, 1) * Z), torch.empty(max(item_cap, 1) * Z, dtype=torch.float64, device="cuda"))
        select_keep.append(out)
        ptrs = [x.data_ptr() for x in out]
        # threshold 0: every listed row of an energy table, every non-negative power
        return lambda: acc.select_above(table, 0, 0, rows[kind], 0, min(item_cap, n), *ptrs, s)

    tables = {"proc": "proc_power", "pod": "pod_energy"}
    select_ms = {k: {"all_outputs": timed(select_call(tables[k], k, kinds[k][1])),
                     "sizing_call": timed(select_call(tables[k], k, 0))} for k in kinds}

    decades_uw = np.array([10.0 ** k for k in range(-2, 13)], dtype=np.float64).view(np.uint64)  # 10 nW .. 1 MW
    decades_uj = np.array([10 ** k for k in range(0, 15)], dtype=np.uint64)                       # 1 µJ .. 100 MJ
    node_of_row = np.repeat(np.arange(N), np.diff(np.asarray(a["proc_off"], dtype=np.int64)))
    cases = [("proc", 1, None, "none (group NULL)")]
    cases += [("proc", g, rng.integers(0, g, P), "random") for g in (8, 1000)]
    cases.append(("proc", 10000, node_of_row % 10000, "per node"))
    cases.append(("proc", 65536, rng.integers(0, 65536, P), "random"))
    cases.append(("pod", L.n_namespaces, L.pod_ns, "namespace"))
    results = []
    for kind, n_groups, group, ids in cases:
        n = kinds[kind][1]
        table = tables[kind]
        bounds = decades_uw if kind == "proc" else decades_uj
        ids_u32 = np.zeros(n, dtype=np.uint32) if group is None else np.ascontiguousarray(group, dtype=np.uint32)
        d_ids = torch.from_numpy(ids_u32.view(np.int32)).cuda()
        call, out = hist_call(table, kind, None if group is None else d_ids, n_groups, bounds)
        ms, all_ms = timed(call)
        gcall, gout = group_call(kind, d_ids, n_groups)
        gms, gall = timed(gcall)
        copies, passes = regime_of(n_groups, len(bounds))
        gpasses = group_passes_of(n_groups, Z)
        id_bytes = 0 if group is None else 4
        per_row = 4 + id_bytes + 8 if passes == 1 else 28 + 4 * passes + 12
        record = 8 * Z + (8 * Z if kind == "pod" else 8)
        group_per_row = 4 + 4 + record if gpasses == 1 else 16 + 4 * gpasses + 12 + record
        binned = int(out[1].view(n_groups, -1)[:, -1].sum().item())
        sum_equal = bool(torch.equal(out[2], (gout[2] if kind == "proc" else gout[1]).view(n_groups, Z)[:, 0].contiguous()))
        count_equal = bool(torch.equal(out[1].view(n_groups, -1)[:, -1] + out[3], gout[0].long()))
        r = {"call": "kacc_group_hist", "table": table, "zone": 0, "rows": n, "n_groups": n_groups, "ids": ids,
             "n_bounds": len(bounds), "lds_copies": copies, "passes": passes, "ms": ms,
             "algorithmic_bytes_per_row": per_row, "algorithmic_bytes": n * per_row, "GBps": n * per_row / ms / 1e6,
             "frac_of_8TBps_spec": n * per_row / ms / 1e6 / HBM_SPEC_GBPS, "rows_binned": binned,
             "nonempty_bins": int((out[0] != 0).sum().item()),
             "group_sums_ms": gms, "group_sums_passes": gpasses, "group_sums_bytes_per_row": group_per_row,
             "ratio_to_group_sums": ms / gms,
             "select_above_all_outputs_ms": select_ms[kind]["all_outputs"][0],
             "ratio_to_select_above_all_outputs": ms / select_ms[kind]["all_outputs"][0],
             "select_above_sizing_call_ms": select_ms[kind]["sizing_call"][0],
             "ratio_to_select_above_sizing_call": ms / select_ms[kind]["sizing_call"][0],
             "sum_equals_group_sums": sum_equal, "count_plus_nan_equals_group_sums": count_equal,
             "all_ms": all_ms, "group_sums_all_ms": gall}
        results.append(r)
        print(json.dumps(r), flush=True)
    acc.sync(s)
    acc.close()
    doc = {
        "bench": "tools/bench_hist.py", "config": 3, "nodes": N, "processes": P, "pods": Q, "zones": Z,
        "namespaces": L.n_namespaces, "calls": args.calls, "reps": args.reps, "warmup": args.warmup,
        "device": torch.cuda.get_device_name(0),
        "method": "one HIP event pair around `calls` back-to-back calls after `warmup` calls; ms per call = window / "
                  "calls; median of `reps` windows",
        "bytes": "per row, one pass: slot word 4 + group id 4 (0 with group NULL) + value 8 (the ratio of a derived "
                 "power, else the table's word of the zone); several passes: 28 (classify: slot word, id and value "
                 "read, row word 4 and sum word 8 written) + 4 x passes (row words) + 12 (owning pass: row word and "
                 "sum word); the accumulator and the outputs are not counted",
        "bounds": {"proc_power": "10^-2 .. 10^12 µW, 15 decades", "pod_energy": "10^0 .. 10^14 µJ, 15 decades"},
        "yardsticks": {"group_sums": "the same ids (zeros for group NULL), every output",
                       "select_above": "threshold 0 on the same table and zone; every output with item_cap = rows, "
                                       "and the sizing call (item_cap 0)",
                       "select_above_all_ms": {k: {m: v[1] for m, v in d.items()} for k, d in select_ms.items()}},
        "cases": results,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": args.out}))


if __name__ == "__main__":
    main()
