#!/usr/bin/env python3
"""Top-K of the live fleet at config 3 (10k nodes x 2k processes, Z = 4) on one MI355X:
kacc_top_nodes / kacc_top_fleet against what a caller had to do without them — scrape the whole
table (kacc_table_read), gather the batch's slots' zone column, torch.topk (per node: a topk
over the [nodes, rows per node] view; config 3's nodes are all the same size, so the baseline
pays no padding).

A fresh interval runs before every timed repetition (the ~240 MB a selection reads would
otherwise sit in the 256 MiB Infinity Cache from the repetition before); one HIP event pair
around the call alone; median of --reps repetitions after --warmup.  Algorithmic bytes of a
selection: 12 B per row (slot word + ratio, or + the stored word) plus its outputs.  Writes
one JSON object to --out and prints it.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_SPEC_GBPS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=0, help="nodes of the config 3 fleet (0: 10000)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--zone", type=int, default=0)
    ap.add_argument("--out", default=os.path.join("profiles", "top", "bench_top.json"))
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
    # two distinct process inputs, fresh node inputs (clock, counters, usage ratio) every step
    prime = to_device(sim.next_interval())
    acc.run_interval(interval_from_tensors(prime, sizes, flags), s)
    full = [to_device(sim.next_interval()) for _ in range(2)]
    node_names = ("node_ts_ns", "node_usage_ratio", "node_status", "zone_energy", "zone_max")
    step_no = [0]
    keep = []

    def fresh_interval():
        k = step_no[0]
        step_no[0] += 1
        t = dict(full[k % 2])
        if k >= 2:
            t.update(to_device({n: a for n, a in sim.next_node_inputs().items() if n in node_names}))
        keep[:] = [t]
        acc.run_interval(interval_from_tensors(t, sizes, flags), s)
        return t

    def timed(call):
        ms = []
        for rep in range(args.warmup + args.reps):
            t = fresh_interval()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = call(t)
            e1.record()
            e1.synchronize()
            if rep >= args.warmup:
                ms.append(e0.elapsed_time(e1))
        acc.sync(s)
        return float(np.median(ms)), ms, out

    kinds = {"proc": (accel.KACC_KIND_PROC, P), "pod": (accel.KACC_KIND_POD, Q)}
    slot_index = {kind: (full[0][f"{kind}_slot"].long() & accel.KACC_SLOT_MASK) for kind in kinds}
    scrape = {kind: torch.empty(max(n, 1) * Z, dtype=torch.float64, device="cuda") for kind, (_, n) in kinds.items()}
    per_node = P // N if N and P % N == 0 else 0
    zone = args.zone

    def new_call(table, k, fleet_call):
        kind = table.split("_")[0]
        lists = 1 if fleet_call else N
        count = torch.empty(lists, dtype=torch.int32, device="cuda")
        row = torch.empty(lists * k, dtype=torch.int32, device="cuda")
        slot = torch.empty(lists * k, dtype=torch.int32, device="cuda")
        node = torch.empty(lists * k, dtype=torch.int32, device="cuda")
        value = torch.empty(lists * k, dtype=torch.int64, device="cuda")

        def call(t):
            rows = top_rows_from_tensors(t, kinds[kind][0])
            if fleet_call:
                acc.top_fleet(table, zone, k, rows, count.data_ptr(), row.data_ptr(), slot.data_ptr(),
                              node.data_ptr(), value.data_ptr(), s)
            else:
                acc.top_nodes(table, zone, k, rows, count.data_ptr(), row.data_ptr(), slot.data_ptr(),
                              value.data_ptr(), s)
            return value
        return call

    def baseline(table, k, fleet_call):
        kind = table.split("_")[0]
        n = kinds[kind][1]

        def call(t):
            acc.read(table, scrape[kind].data_ptr(), 0, n * Z, s)
            col = scrape[kind].view(-1, Z)[slot_index[kind], zone]
            if fleet_call:
                return torch.topk(col, min(k, n)).values
            return torch.topk(col.view(N, per_node), min(k, per_node), dim=1).values
        return call

    cases = [("top_nodes", "proc_power", 10), ("top_nodes", "proc_power", 100),
             ("top_fleet", "proc_power", 100), ("top_fleet", "proc_power", 1024), ("top_fleet", "pod_power", 100)]
    results = []
    for fn, table, k in cases:
        fleet_call = fn == "top_fleet"
        if not fleet_call and not per_node:
            continue
        n = kinds[table.split("_")[0]][1]
        ms, all_ms, value = timed(new_call(table, k, fleet_call))
        base_ms, base_all, want = timed(baseline(table, k, fleet_call))
        # the timed runs each followed their own interval: compare the two on one more snapshot
        t = fresh_interval()
        got = new_call(table, k, fleet_call)(t).view(torch.float64)
        ref = baseline(table, k, fleet_call)(t)
        acc.sync(s)
        kk = ref.shape[-1]
        got = got.view(-1, k)[:, :kk].reshape(ref.shape)
        match = bool(torch.equal(got, ref))
        out_bytes = (4 + k * 20) if fleet_call else N * (4 + k * 16)
        nbytes = 12 * n + out_bytes
        results.append({
            "call": f"kacc_{fn}", "table": table, "k": k, "zone": zone, "rows": n,
            "ms": ms, "baseline_ms": base_ms, "speedup": base_ms / ms if ms > 0 else None,
            "faster_than_baseline": ms < base_ms,
            "algorithmic_bytes": nbytes, "GBps": nbytes / ms / 1e6, "frac_of_8TBps_spec": nbytes / ms / 1e6 / HBM_SPEC_GBPS,
            "values_equal_baseline": match, "all_ms": all_ms, "baseline_all_ms": base_all,
        })
        print(json.dumps(results[-1]), flush=True)
    acc.close()
    doc = {
        "bench": "tools/bench_top.py", "config": 3, "nodes": N, "processes": P, "pods": Q, "zones": Z,
        "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
        "method": "a fresh interval before every repetition; one HIP event pair around the call; median",
        "baseline": "kacc_table_read of the whole table + gather of the batch's slots' zone column + torch.topk "
                    "(per node: topk over the [nodes, rows per node] view)",
        "cases": results,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": args.out, "all_faster": all(r["faster_than_baseline"] for r in results)}))


if __name__ == "__main__":
    main()
