#!/usr/bin/env python3
"""Exact quantiles of the running workloads at config 3 (10k nodes x 2k processes, 700k pods in
10,000 namespaces, Z = 4) on one MI355X: kacc_group_quantiles with every output on, for the process
power of zone 0 with 1 group (group NULL), 8, 1000 and 65 536 random groups and 10 000 per-node
groups, each with n_phi 1 ([0.99]; [1.0] for the one-group case) and 3 ([0.5, 0.9, 0.99]), and for
the pod energy by namespace.

Yardsticks, measured in the same run on the same box and reported as ratios (the parent commit has
no counterpart, so nothing is gated on an absolute time): kacc_group_hist with 15 decade bounds on
the same ids and table, and kacc_top_fleet(k = 1) for the one-group, phi = 1 case.

The unit's two tuning knobs are measured here too (--knobs): KACC_QUANT_LDS_QUERIES (the largest
n_groups * n_phi whose counters live in LDS; 0 forces the global counters) on the cases that fit
LDS, and KACC_QUANT_MERGE_ROUNDS (the wave merges before the plain atomic) on the cases that do not.

One HIP event pair around --calls back-to-back calls after --warmup calls; ms per call is the
window over the calls; the median of --reps windows.
Algorithmic bytes of a call, per row: 28 for the key pass (slot word 4, group id 4 - none with
group NULL -, value 8 read; key 8 and group word 4 written), 12 for each of the eight digit passes
and 12 for the successor pass (the row records); the queries' prefixes and the counters (L2
resident up to a few thousand queries) and the outputs are not counted.
Writes one JSON object to --out and prints it.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_SPEC_GBPS = 8000.0
DIGITS, LDS_WORDS, MAX_COPIES = 256, 16384, 64  # kacc_quant.hip: kDigits, kLdsWords, rows::kMaxCopies


def regime_of(n_groups, n_phi, lds_queries=LDS_WORDS // DIGITS):
    """(where, copies) kacc_quant.hip counts with."""
    q = n_groups * n_phi
    if q > lds_queries:
        return "global", 0
    words, copies = q * DIGITS, 1
    if 2 * (words | 1) <= LDS_WORDS:
        while copies < MAX_COPIES and 2 * copies * (words | 1) <= LDS_WORDS:
            copies *= 2
    return "lds", copies


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=0, help="nodes of the config 3 fleet (0: 10000)")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--knobs", action="store_true", help="also time the regime and merge-round variants")
    ap.add_argument("--out", default=os.path.join("profiles", "quant", "bench.json"))
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

    def timed_with(env, call):
        old = {k: os.environ.get(k) for k in env}
        os.environ.update({k: str(v) for k, v in env.items()})
        try:
            return timed(call)
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v

    kinds = {"proc": (accel.KACC_KIND_PROC, P), "pod": (accel.KACC_KIND_POD, Q)}
    rows = {k: top_rows_from_tensors(t, kinds[k][0]) for k in kinds}
    rng = np.random.default_rng(1)
    i64 = lambda n: torch.empty(n, dtype=torch.int64, device="cuda")  # noqa: E731

    def quant_call(table, kind, d_group, n_groups, phi):
        q = n_groups * len(phi)
        out = (i64(n_groups), i64(n_groups), i64(q), i64(q), i64(q), i64(q))
        ptrs = [x.data_ptr() for x in out]

        def call():
            acc.group_quantiles(table, 0, rows[kind], d_group.data_ptr() if d_group is not None else 0, n_groups, phi,
                                0, *ptrs, s)
        return call, out

    def hist_call(table, kind, d_group, n_groups, bounds):
        b1 = len(bounds) + 1
        out = (i64(n_groups * b1), i64(n_groups * b1), i64(n_groups), i64(n_groups), i64(n_groups))
        ptrs = [x.data_ptr() for x in out]

        def call():
            acc.group_hist(table, 0, rows[kind], d_group.data_ptr() if d_group is not None else 0, n_groups, bounds, 0,
                           *ptrs, s)
        return call

    top_out = (torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"),
               torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"), i64(1))
    top_ms = timed(lambda: acc.top_fleet("proc_power", 0, 1, rows["proc"], *(x.data_ptr() for x in top_out), s))

    # the share of the fleet's process powers of zone 0 that are exactly 0: with one group they all
    # hit one counter, the worst case for contention
    buf = torch.empty(acc.table_info("proc_power")[1], dtype=torch.float64, device="cuda")
    acc.read("proc_power", buf.data_ptr(), stream=s)
    acc.sync(s)
    slots = (torch.from_numpy((np.asarray(a["proc_slot"]) & np.uint32(accel.KACC_SLOT_MASK)).astype(np.int64))).cuda()
    zero_share = float((buf.view(-1, Z)[slots, 0] == 0).double().mean().item())
    del buf

    decades_uw = np.array([10.0 ** k for k in range(-2, 13)], dtype=np.float64).view(np.uint64)  # 10 nW .. 1 MW
    decades_uj = np.array([10 ** k for k in range(0, 15)], dtype=np.uint64)                       # 1 µJ .. 100 MJ
    node_of_row = np.repeat(np.arange(N), np.diff(np.asarray(a["proc_off"], dtype=np.int64)))
    tables = {"proc": "proc_power", "pod": "pod_energy"}
    cases = [("proc", 1, None, "none (group NULL)")]
    cases += [("proc", g, rng.integers(0, g, P), "random") for g in (8, 1000)]
    cases.append(("proc", 10000, node_of_row % 10000, "per node"))
    cases.append(("proc", 65536, rng.integers(0, 65536, P), "random"))
    cases.append(("pod", L.n_namespaces, L.pod_ns, "namespace"))
    results = []
    for kind, n_groups, group, ids in cases:
        n = kinds[kind][1]
        table = tables[kind]
        ids_u32 = np.zeros(n, dtype=np.uint32) if group is None else np.ascontiguousarray(group, dtype=np.uint32)
        d_ids = torch.from_numpy(ids_u32.view(np.int32)).cuda()
        d_group = None if group is None else d_ids
        hms, hall = timed(hist_call(table, kind, d_group, n_groups, decades_uw if kind == "proc" else decades_uj))
        for phi in (([1.0] if n_groups == 1 else [0.99]), [0.5, 0.9, 0.99]):
            if n_groups * len(phi) > accel.KACC_QUANT_MAX_QUERIES:
                continue
            call, out = quant_call(table, kind, d_group, n_groups, phi)
            ms, all_ms = timed(call)
            where, copies = regime_of(n_groups, len(phi))
            per_row = 12 + (0 if group is None else 4) + 12 + 12 * 8 + 12
            r = {"call": "kacc_group_quantiles", "table": table, "zone": 0, "rows": n, "n_groups": n_groups, "ids": ids,
                 "phi": phi, "queries": n_groups * len(phi), "counters": where, "lds_copies": copies, "ms": ms,
                 "algorithmic_bytes_per_row": per_row, "algorithmic_bytes": n * per_row, "GBps": n * per_row / ms / 1e6,
                 "frac_of_8TBps_spec": n * per_row / ms / 1e6 / HBM_SPEC_GBPS,
                 "rows_ranked": int(out[0].sum().item()), "rows_nan": int(out[1].sum().item()),
                 "group_hist_15_bounds_ms": hms, "ratio_to_group_hist": ms / hms, "all_ms": all_ms,
                 "group_hist_all_ms": hall}
            if kind == "proc":
                r["share_of_rows_exactly_zero"] = zero_share
            if n_groups == 1 and phi == [1.0]:
                r["top_fleet_k1_ms"] = top_ms[0]
                r["ratio_to_top_fleet_k1"] = ms / top_ms[0]
                r["max_equals_top_fleet"] = bool(out[2][0].item() == top_out[4][0].item())
            if args.knobs:
                if where == "lds":
                    g_ms, g_all = timed_with({"KACC_QUANT_LDS_QUERIES": 0}, call)
                    r["forced_global_counters_ms"] = g_ms
                    r["forced_global_counters_all_ms"] = g_all
                    r["forced_global_no_merge_ms"] = timed_with({"KACC_QUANT_LDS_QUERIES": 0,
                                                                 "KACC_QUANT_MERGE_ROUNDS": 0}, call)[0]
                else:
                    r["merge_rounds_ms"] = {str(m): timed_with({"KACC_QUANT_MERGE_ROUNDS": m}, call)[0]
                                            for m in (0, 1, 2, 4, 8)}
            results.append(r)
            print(json.dumps(r), flush=True)
    acc.sync(s)
    acc.close()
    doc = {
        "bench": "tools/bench_quant.py", "config": 3, "nodes": N, "processes": P, "pods": Q, "zones": Z,
        "namespaces": L.n_namespaces, "calls": args.calls, "reps": args.reps, "warmup": args.warmup,
        "device": torch.cuda.get_device_name(0),
        "method": "one HIP event pair around `calls` back-to-back calls after `warmup` calls; ms per call = window / "
                  "calls; median of `reps` windows",
        "bytes": "per row: key pass 12 read (slot word 4, value 8; + group id 4 with ids) + 12 written (key 8, group "
                 "word 4); 12 for each of the eight digit passes; 12 for the successor pass; the prefixes, the "
                 "counters and the outputs are not counted",
        "share_of_process_powers_exactly_zero": zero_share,
        "yardsticks": {"group_hist": "the same ids and table, 15 decade bounds, every output",
                       "top_fleet": "kacc_top_fleet(k = 1) on proc_power, zone 0, every output",
                       "top_fleet_all_ms": top_ms[1]},
        "cases": results,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": args.out}))


if __name__ == "__main__":
    main()
