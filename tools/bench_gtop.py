#!/usr/bin/env python3
"""Top-K running workloads per group at config 3 (10k nodes x 2k processes, 700k pods in 10,000
namespaces, Z = 4) on one MI355X: kacc_group_top with every output on, for the process power of
zone 0 with 1 group (group NULL, k 100), 8 random groups (k 10), 1000 random groups (k 10 and 100),
10 000 per-node groups (k 10 and 100) and 65 536 random groups (k 16), and for the pod power by
namespace (k 5).

Yardsticks, measured in the same run on the same box and reported as ratios (the parent commit has
no counterpart, so nothing is gated on an absolute time):
  - kacc_group_quantiles with one phi on the same ids and table (the same pass structure);
  - kacc_top_fleet for the one-group case and kacc_top_nodes for the per-node ids (the specialised
    calls; the header points to them where they apply);
  - the alternative the call replaces: kacc_table_read of the whole table, a gather of the batch's
    slots' zone column and a torch sort by (group, key descending, row) on the device.
The lists' values and counts must equal that sort's, bit for bit (asserted: at 20 M rows this is
the only check in which the fourth digit of the row index takes part in a tie cut).

The unit's knobs are measured too (--knobs): KACC_GTOP_LDS_GROUPS (0 forces the global counters)
on the cases that fit LDS, KACC_GTOP_MERGE_ROUNDS on the others, KACC_GTOP_ROW_EXIT (0: the row
passes walk the records although no group has a cut block of equal keys).

One HIP event pair around --calls back-to-back calls after --warmup calls; ms per call is the
window over the calls; the median of --reps windows.
Algorithmic bytes of a call, per row: 24 for the key pass (slot word 4, value 8 read; ~key 8 and
group word 4 written; + 4 with group ids), 12 for each of the eight key digit passes and 12 for
the emit pass (the row records).  The row digit passes (they return at once unless a block of
equal keys is cut), the counters, the groups' state, the segments and the outputs are not counted.
Writes one JSON object to --out and prints it.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_SPEC_GBPS = 8000.0
DIGITS, LDS_WORDS, MAX_COPIES = 256, 16384, 64  # kacc_gtop.hip: kDigits, kLdsWords, rows::kMaxCopies


def regime_of(n_groups):
    """(where, copies) kacc_gtop.hip counts with."""
    if n_groups > LDS_WORDS // DIGITS:
        return "global", 0
    words, copies = n_groups * DIGITS, 1
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
    ap.add_argument("--knobs", action="store_true", help="also time the regime, merge-round and row-exit variants")
    ap.add_argument("--out", default=os.path.join("profiles", "gtop", "bench.json"))
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

    def timed(call, calls=args.calls):
        for _ in range(args.warmup):
            call()
        acc.sync(s)
        ms = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                call()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / calls)
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
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device="cuda")  # noqa: E731
    i64 = lambda n: torch.empty(n, dtype=torch.int64, device="cuda")  # noqa: E731
    MIN = torch.iinfo(torch.int64).min

    def host_alternative(table, kind, d_ids, n_groups, k):
        """What the call replaces, on the device with torch: (call, result()) - result() gives the
        count [G] and the value bits [G, k] of the lists."""
        n = kinds[kind][1]
        buf = torch.empty(acc.table_info(table)[1], dtype=torch.float64, device="cuda")
        words = np.asarray(a[f"{kind}_slot"])
        slots = torch.from_numpy((words & np.uint32(accel.KACC_SLOT_MASK)).astype(np.int64)).cuda()
        off = np.asarray(a[f"{kind}_off"], dtype=np.int64)
        listed = (np.asarray(a["node_status"], dtype=np.uint32) & np.uint32(accel.KACC_NODE_READ_ERROR)) == 0
        row_listed = torch.from_numpy(np.repeat(listed, np.diff(off))).cuda()
        ids = d_ids.to(torch.int64) & 0xFFFFFFFF
        ids = torch.where(row_listed & (ids < n_groups), ids, torch.full_like(ids, n_groups))  # left out: sorted last
        keep = {}

        def call():
            acc.read(table, buf.data_ptr(), stream=s)
            v = buf.view(-1, Z)[slots, 0]
            b = v.view(torch.int64)
            key = torch.where(b < 0, ~b, b | MIN)
            key = torch.where(v == 0, torch.full_like(key, MIN), key)
            key = torch.where(v != v, torch.zeros_like(key), key)
            by_key = torch.argsort(~key ^ MIN, stable=True)  # descending u64 key, equal keys by ascending row
            order = by_key[torch.argsort(ids[by_key], stable=True)]
            keep["order"], keep["bits"], keep["key"] = order, b, key

        def result():
            order, b = keep["order"], keep["bits"]
            g = ids[order]
            cnt = torch.bincount(g, minlength=n_groups + 1)[:n_groups]
            start = torch.cumsum(cnt, 0) - cnt
            ok = g < n_groups
            place = torch.arange(n, device="cuda")[ok] - start[g[ok]]
            take = place < k
            values = torch.zeros(n_groups * k, dtype=torch.int64, device="cuda")
            values[g[ok][take] * k + place[take]] = b[order[ok][take]]
            # groups whose list ends inside a block of equal keys: their cut is by row index
            key_sorted = keep["key"][order[ok]]
            last = (place == k - 1) & (cnt[g[ok]] > k)
            at = torch.nonzero(last).reshape(-1)
            cut = int((key_sorted[at] == key_sorted[at + 1]).sum().item())
            return torch.clamp(cnt, max=k), values, cut
        return call, result

    node_of_proc = np.repeat(np.arange(N), np.diff(np.asarray(a["proc_off"], dtype=np.int64)))
    cases = [("proc", 1, None, "none (group NULL)", 100)]
    cases.append(("proc", 8, rng.integers(0, 8, P), "random", 10))
    ids_1000 = rng.integers(0, 1000, P)
    cases += [("proc", 1000, ids_1000, "random", k) for k in (10, 100)]
    cases += [("proc", N, node_of_proc, "per node", k) for k in (10, 100)]
    cases.append(("proc", 65536, rng.integers(0, 65536, P), "random", 16))
    cases.append(("pod", L.n_namespaces, L.pod_ns, "namespace", 5))
    tables = {"proc": "proc_power", "pod": "pod_power"}
    results = []
    for kind, n_groups, group, ids, k in cases:
        n = kinds[kind][1]
        table = tables[kind]
        ids_u32 = np.zeros(n, dtype=np.uint32) if group is None else np.ascontiguousarray(group, dtype=np.uint32)
        d_ids = torch.from_numpy(ids_u32.view(np.int32)).cuda()
        d_group = None if group is None else d_ids
        gp = d_group.data_ptr() if d_group is not None else 0
        out = (i32(n_groups), i32(n_groups * k), i32(n_groups * k), i32(n_groups * k), i64(n_groups * k))
        ptrs = [x.data_ptr() for x in out]

        def call():
            acc.group_top(table, 0, k, rows[kind], gp, n_groups, 0, *ptrs, s)

        ms, all_ms = timed(call)
        q_out = [i64(n_groups) for _ in range(6)]
        q_ms, q_all = timed(lambda: acc.group_quantiles(table, 0, rows[kind], gp, n_groups, [0.99], 0,
                                                        *(x.data_ptr() for x in q_out), s))
        alt, alt_result = host_alternative(table, kind, d_ids, n_groups, k)
        alt_ms, alt_all = timed(alt, calls=3)
        want_count, want_values, cut_groups = alt_result()
        call()
        acc.sync(s)
        equal = bool(torch.equal(out[0].to(torch.int64), want_count) and torch.equal(out[4], want_values))
        assert equal, f"{table} G{n_groups} k{k}: the lists differ from the torch sort"
        where, copies = regime_of(n_groups)
        per_row = 12 + (0 if group is None else 4) + 12 + 12 * 8 + 12
        r = {"call": "kacc_group_top", "table": table, "zone": 0, "rows": n, "n_groups": n_groups, "ids": ids, "k": k,
             "counters": where, "lds_copies": copies, "sort": "wave" if k <= 64 else "workgroup", "ms": ms,
             "algorithmic_bytes_per_row": per_row, "algorithmic_bytes": n * per_row, "GBps": n * per_row / ms / 1e6,
             "frac_of_8TBps_spec": n * per_row / ms / 1e6 / HBM_SPEC_GBPS,
             "rows_listed": int(out[0].sum().item()), "groups_cut_inside_equal_keys": cut_groups,
             "row_digit_passes": int(max(0, (int(n - 1).bit_length() + 7) // 8)),
             "values_and_counts_equal_torch_sort": equal,
             "group_quantiles_1_phi_ms": q_ms, "ratio_to_group_quantiles": ms / q_ms,
             "read_gather_torch_sort_ms": alt_ms, "speedup_over_read_gather_sort": alt_ms / ms,
             "all_ms": all_ms, "group_quantiles_all_ms": q_all, "read_gather_torch_sort_all_ms": alt_all}
        if group is None:
            f_ms, f_all = timed(lambda: acc.top_fleet(table, 0, k, rows[kind], *ptrs, s))
            r.update({"top_fleet_ms": f_ms, "ratio_to_top_fleet": ms / f_ms, "top_fleet_all_ms": f_all})
        if ids == "per node":
            n_ms, n_all = timed(lambda: acc.top_nodes(table, 0, k, rows[kind], ptrs[0], ptrs[1], ptrs[2], ptrs[4], s))
            r.update({"top_nodes_ms": n_ms, "ratio_to_top_nodes": ms / n_ms, "top_nodes_all_ms": n_all})
        if args.knobs:
            r["row_passes_not_skipped_ms"] = timed_with({"KACC_GTOP_ROW_EXIT": 0}, call)[0]
            if where == "lds":
                r["forced_global_counters_ms"] = timed_with({"KACC_GTOP_LDS_GROUPS": 0}, call)[0]
            else:
                r["merge_rounds_ms"] = {str(m): timed_with({"KACC_GTOP_MERGE_ROUNDS": m}, call)[0] for m in (0, 4, 8)}
        results.append(r)
        print(json.dumps(r), flush=True)
        del out, q_out, alt, alt_result, want_count, want_values
        torch.cuda.empty_cache()
    acc.sync(s)
    acc.close()
    doc = {
        "bench": "tools/bench_gtop.py", "config": 3, "nodes": N, "processes": P, "pods": Q, "zones": Z,
        "namespaces": L.n_namespaces, "calls": args.calls, "reps": args.reps, "warmup": args.warmup,
        "device": torch.cuda.get_device_name(0),
        "method": "one HIP event pair around `calls` back-to-back calls after `warmup` calls; ms per call = window / "
                  "calls; median of `reps` windows (the torch alternative: 3 calls per window)",
        "bytes": "per row: key pass 12 read (slot word 4, value 8; + group id 4 with ids) + 12 written (~key 8, group "
                 "word 4); 12 for each of the eight key digit passes; 12 for the emit pass; the row digit passes, the "
                 "counters, the groups' state, the segments and the outputs are not counted",
        "yardsticks": {"group_quantiles": "the same ids and table, phi = [0.99], every output",
                       "top_fleet / top_nodes": "the same table, zone and k, every output",
                       "read_gather_torch_sort": "kacc_table_read of the table, gather of (slot, zone 0), the sort key, two "
                                                 "stable torch.argsort (key descending, then group) on the device"},
        "cases": results,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": args.out}))


if __name__ == "__main__":
    main()
