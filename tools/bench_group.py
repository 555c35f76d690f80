#!/usr/bin/env python3
"""Running workloads summed by group at config 3 (10k nodes x 2k processes, Z = 4) on one MI355X:
kacc_group_sums with every output on, for the processes with 8, 1000, 10 000 and 65 536 random
groups and for the pods by namespace.

Yardsticks, measured in the same run on the same box (reported, not gated on; the parent commit
has no counterpart): kacc_select_above at threshold 0 with every output (the project's existing
pass over the same rows and records) and, for the pods, kacc_namespace_totals.

One HIP event pair around --calls back-to-back calls after --warmup calls; ms per call is the
window over the calls; the median of --reps windows.  The rows' records (about 1 GB for the
processes) exceed the 256 MiB Infinity Cache, so back-to-back calls do not serve each other.
Algorithmic bytes of a call, per row: with one pass the slot word (4), the group id (4), the
energy record (8 Z) and the ratio (8; a pod: the stored power record, 8 Z); with several passes
16 for the classify pass, 4 per pass for the row words, 12 in the owning pass and the record.
Writes one JSON object to --out and prints it.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_SPEC_GBPS = 8000.0
SMALL_WORDS, BIG_WORDS, PASS_WORDS = 4096, 9984, 9728  # kacc_group.hip: kSmallWords, kBigWords, kPassWords


def passes_of(n_groups, zones):
    """The pass count kacc_group.hip runs for this many groups."""
    w = 1 + 2 * zones
    if ((n_groups * w) | 1) <= SMALL_WORDS or n_groups * w <= BIG_WORDS:
        return 1
    bins = PASS_WORDS // w
    return (n_groups + bins - 1) // bins


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=0, help="nodes of the config 3 fleet (0: 10000)")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "group", "bench.json"))
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
    t = None
    for _ in range(2):  # the second interval has powers
        t = to_device(sim.next_interval())
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

    def group_call(kind, group, n_groups):
        d_group = torch.from_numpy(np.ascontiguousarray(group, dtype=np.uint32).view(np.int32)).cuda()
        cnt = torch.empty(n_groups, dtype=torch.int32, device="cuda")
        drp = torch.empty(n_groups, dtype=torch.int32, device="cuda")
        e, fx = (torch.empty(n_groups * Z, dtype=torch.int64, device="cuda") for _ in range(2))
        p = torch.empty(n_groups * Z, dtype=torch.float64, device="cuda")

        def call():
            acc.group_sums(kinds[kind][0], rows[kind], d_group.data_ptr(), n_groups, 0, cnt.data_ptr(), e.data_ptr(),
                           fx.data_ptr(), p.data_ptr(), drp.data_ptr(), s)
        return call, (d_group, cnt, e, fx, p, drp)

    select_out = {}

    def select_call(kind):
        n = kinds[kind][1]
        select_out[kind] = (torch.zeros(N + 1, dtype=torch.int32, device="cuda"),
                            *(torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(3)),
                            torch.empty(n * Z, dtype=torch.int64, device="cuda"),
                            torch.empty(n * Z, dtype=torch.float64, device="cuda"))
        ptrs = [x.data_ptr() for x in select_out[kind]]

        def call():
            acc.select_above(f"{kind}_energy", 0, 0, rows[kind], 0, n, *ptrs, s)
        return call

    select_ms = {kind: timed(select_call(kind)) for kind in kinds}
    off, slots = L.namespace_csr()
    d_csr = to_device({"o": off, "s": slots})
    ns_e = torch.empty(L.n_namespaces * Z, dtype=torch.int64, device="cuda")
    ns_p = torch.empty(L.n_namespaces * Z, dtype=torch.float64, device="cuda")
    ns_ms = timed(lambda: acc.namespace_totals(L.n_namespaces, d_csr["o"].data_ptr(), d_csr["s"].data_ptr(),
                                               ns_e.data_ptr(), ns_p.data_ptr(), s))

    cases = [("proc", g, rng.integers(0, g, P)) for g in (8, 1000, 10000, 65536)]
    cases.append(("pod", L.n_namespaces, L.pod_ns))
    results = []
    for kind, n_groups, group in cases:
        n = kinds[kind][1]
        call, keep = group_call(kind, group, n_groups)
        ms, all_ms = timed(call)
        passes = passes_of(n_groups, Z)
        record = 8 * Z + (8 * Z if kind == "pod" else 8)
        # several passes: the rows pass reads slot word and id and writes the row word and node (16 B), every
        # pass reads the row words, the owning pass reads slot word, node and row word again (12 B)
        nbytes = n * (4 + 4 + record) if passes == 1 else n * (16 + 4 * passes + 12 + record)
        counted = int(keep[1].long().sum().item())
        r = {"call": "kacc_group_sums", "kind": kind, "rows": n, "n_groups": n_groups, "passes": passes,
             "ms": ms, "algorithmic_bytes": nbytes, "GBps": nbytes / ms / 1e6,
             "frac_of_8TBps_spec": nbytes / ms / 1e6 / HBM_SPEC_GBPS, "rows_counted": counted,
             "select_above_all_outputs_ms": select_ms[kind][0], "ratio_to_select_above": ms / select_ms[kind][0],
             "all_ms": all_ms}
        if kind == "pod":
            r["namespace_totals_ms"] = ns_ms[0]
            r["ratio_to_namespace_totals"] = ms / ns_ms[0]
            r["energy_equals_namespace_totals"] = bool(torch.equal(keep[2], ns_e))
        results.append(r)
        print(json.dumps(r), flush=True)
    acc.sync(s)
    acc.close()
    doc = {
        "bench": "tools/bench_group.py", "config": 3, "nodes": N, "processes": P, "pods": Q, "zones": Z,
        "namespaces": L.n_namespaces, "calls": args.calls, "reps": args.reps, "warmup": args.warmup,
        "device": torch.cuda.get_device_name(0),
        "method": "one HIP event pair around `calls` back-to-back calls after `warmup` calls; ms per call = window / "
                  "calls; median of `reps` windows",
        "bytes": "per row, one pass: slot word 4 + group id 4 + energy record 8 Z + ratio 8 (pods: stored power "
                 "record 8 Z); several passes: 16 (classify: slot word, id, row word and node written) + 4 x passes "
                 "(row words) + 12 (owning pass: slot word, node, row word) + the record; the accumulator and the "
                 "outputs (n_groups x (8 + 16 Z) each way) are not counted",
        "yardsticks": {"select_above": "threshold 0 on the kind's energy table, every output, item_cap = rows",
                       "select_above_all_ms": {k: v[1] for k, v in select_ms.items()},
                       "namespace_totals_all_ms": ns_ms[1]},
        "cases": results,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": args.out}))


if __name__ == "__main__":
    main()
