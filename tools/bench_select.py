#!/usr/bin/env python3
"""Running workloads above a threshold at config 3 (10k nodes x 2k processes, Z = 4) on one
MI355X: kacc_select_above with every output on, against what a caller had to do without it —
scrape the kind's energy and power tables whole (kacc_table_read), gather the batch slots' zone
column, a torch boolean mask + nonzero, and a row gather of both tables.

The thresholds are taken from the data (the k-th largest power of one snapshot) to select about
1 %, 10 % and 50 % of the rows; the share each timed call really selected is recorded.  A fresh
interval runs before every timed repetition (what the call reads would otherwise sit in the
256 MiB Infinity Cache from the repetition before); one HIP event pair around the call alone;
median of --reps repetitions after --warmup.  Algorithmic bytes of a selection: 12 B per row
(slot word + ratio, or + the stored word) plus, per item, its outputs (12 + 16 Z) and the reads
of its record (8 Z energies; 8 Z more for a stored pod power).  Writes one JSON object to --out
and prints it.
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
    ap.add_argument("--out", default=os.path.join("profiles", "select", "bench.json"))
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
        ms, outs = [], None
        for rep in range(args.warmup + args.reps):
            t = fresh_interval()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            outs = call(t)
            e1.record()
            e1.synchronize()
            if rep >= args.warmup:
                ms.append(e0.elapsed_time(e1))
        acc.sync(s)
        return float(np.median(ms)), ms, outs

    kinds = {"proc": (accel.KACC_KIND_PROC, P), "pod": (accel.KACC_KIND_POD, Q)}
    # the batch slots of the two alternating inputs, by the slot tensor's address
    slot_index = {kind: {b[f"{kind}_slot"].data_ptr(): (b[f"{kind}_slot"].long() & accel.KACC_SLOT_MASK)
                         for b in full} for kind in kinds}
    scrape_e = {kind: torch.empty(max(n, 1) * Z, dtype=torch.int64, device="cuda") for kind, (_, n) in kinds.items()}
    scrape_p = {kind: torch.empty(max(n, 1) * Z, dtype=torch.float64, device="cuda") for kind, (_, n) in kinds.items()}
    zone = args.zone

    def column(kind, t):
        acc.read(f"{kind}_power", scrape_p[kind].data_ptr(), 0, kinds[kind][1] * Z, s)
        return scrape_p[kind].view(-1, Z)[slot_index[kind][t[f"{kind}_slot"].data_ptr()], zone]

    def threshold_for(kind, share):
        """The power the top `share` of the rows of one snapshot reach (a positive f64)."""
        col = column(kind, fresh_interval())
        k = max(1, min(col.numel(), int(round(col.numel() * (1.0 - share)))))
        v = float(torch.kthvalue(col, k).values.item())
        return v if v > 0 else 5e-324

    outputs = {}

    def new_call(table, thr):
        kind = table.split("_")[0]
        n = kinds[kind][1]
        if kind not in outputs:
            outputs[kind] = (torch.zeros(N + 1, dtype=torch.int32, device="cuda"),
                             torch.empty(n, dtype=torch.int32, device="cuda"),
                             torch.empty(n, dtype=torch.int32, device="cuda"),
                             torch.empty(n, dtype=torch.int32, device="cuda"),
                             torch.empty(n * Z, dtype=torch.int64, device="cuda"),
                             torch.empty(n * Z, dtype=torch.float64, device="cuda"))
        off, row, slot, node, e, p = outputs[kind]
        bits = int(np.array([thr], dtype=np.float64).view(np.uint64)[0])

        def call(t):
            rows = top_rows_from_tensors(t, kinds[kind][0])
            acc.select_above(table, zone, bits, rows, 0, n, off.data_ptr(), row.data_ptr(), slot.data_ptr(),
                             node.data_ptr(), e.data_ptr(), p.data_ptr(), s)
            return off, e, p
        return call

    def baseline(table, thr):
        kind = table.split("_")[0]
        n = kinds[kind][1]

        def call(t):
            acc.read(f"{kind}_energy", scrape_e[kind].data_ptr(), 0, n * Z, s)
            col = column(kind, t)  # reads the power table
            sel = torch.nonzero(col >= thr).squeeze(1)
            sl = slot_index[kind][t[f"{kind}_slot"].data_ptr()][sel]
            return sel, scrape_e[kind].view(-1, Z)[sl], scrape_p[kind].view(-1, Z)[sl]
        return call

    cases = [("proc_power", 0.01), ("proc_power", 0.10), ("proc_power", 0.50), ("pod_power", 0.10)]
    results = []
    for table, share in cases:
        kind = table.split("_")[0]
        n = kinds[kind][1]
        thr = threshold_for(kind, share)
        ms, all_ms, (off, _, _) = timed(new_call(table, thr))
        items = int(off[-1].item())
        base_ms, base_all, _ = timed(baseline(table, thr))
        # the timed runs each followed their own interval: compare the two on one more snapshot
        t = fresh_interval()
        off, e, p = new_call(table, thr)(t)
        sel, want_e, want_p = baseline(table, thr)(t)
        acc.sync(s)
        k = int(off[-1].item())
        match = bool(k == sel.numel() and torch.equal(e[: k * Z].view(-1, Z), want_e)
                     and torch.equal(p[: k * Z].view(torch.int64), want_p.reshape(-1).view(torch.int64)))
        stored = kind == "pod"
        nbytes = 12 * n + items * (12 + 16 * Z + 8 * Z + (8 * Z if stored else 12))
        results.append({
            "call": "kacc_select_above", "table": table, "zone": zone, "rows": n, "threshold_uW": thr,
            "target_share": share, "items": items, "share": items / n if n else None,
            "ms": ms, "baseline_ms": base_ms, "speedup": base_ms / ms if ms > 0 else None,
            "faster_than_baseline": ms < base_ms,
            "algorithmic_bytes": nbytes, "GBps": nbytes / ms / 1e6, "frac_of_8TBps_spec": nbytes / ms / 1e6 / HBM_SPEC_GBPS,
            "outputs_equal_baseline": match, "all_ms": all_ms, "baseline_all_ms": base_all,
        })
        print(json.dumps(results[-1]), flush=True)
    acc.close()
    doc = {
        "bench": "tools/bench_select.py", "config": 3, "nodes": N, "processes": P, "pods": Q, "zones": Z,
        "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
        "method": "a fresh interval before every repetition; one HIP event pair around the call; median",
        "baseline": "kacc_table_read of the kind's energy and power tables + gather of the batch slots' zone column "
                    "+ torch mask, nonzero and row gather of both tables",
        "bytes": "12 B per row (slot word + ratio or stored word) + per item 12 + 16 Z of outputs and the reads of "
                 "its record (8 Z energies, + 8 Z stored powers or + 12 B slot word and ratio); the 1-bit-per-row "
                 "mask between the two passes is not counted",
        "cases": results,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": args.out, "all_faster": all(r["faster_than_baseline"] for r in results)}))


if __name__ == "__main__":
    main()
