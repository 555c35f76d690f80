#!/usr/bin/env python3
"""kacc_window_* at config 3 (10k nodes x 2k processes, Z = 4, 2 % churn) on one MI355X.

step   the production interval order under KACC_JOIN_REUSE_TERMINATED with /proc-shaped churn
       (fleet.ProcChurn): join -> tracker add -> window step -> interval on one stream, a HIP event
       between the stages; the median of --steps intervals per stage, so the step's share of the
       interval it is added to, and the tracker's add beside it, come from the same box and run.
       Algorithmic bytes of a step: the slot words (4 per row); per NEW row its id (4), the id
       stored (4) and the base zeroed (8 Z); per terminated slot its list word (4), the exchanged
       id (4 + 4), two records read (16 Z) and one group's words added (8 Z + 4).
       --step-groups / --step-ids / --step-only vary the window of that pipeline: the group count,
       ids that concentrate in a few groups (many of a node's terminated slots then share one),
       and no read cases.  KACC_WINDOW_MERGE_ROUNDS (the library's knob, default 4) sets the wave
       merges of the retire phase where it adds straight into the window's words (more groups
       than LDS holds); 0 turns them off.
read   every output on, for 8, 1000, 10 000 and 65 536 random groups, alternated --reps times
       with kacc_group_sums (every output on) over the same rows and ids (for the group sums of
       another build of the library run tools/bench_group.py under KACC_LIB).
       Algorithmic bytes per row: read: slot word 4 + the slot's id 4 + two records in 16 Z + one
       out 8 Z; group sums: slot word 4 + id 4 + record 8 Z + ratio 8.
mark   the copy: 16 Z bytes per slot.

One HIP event pair around --calls back-to-back calls after --warmup calls; ms per call is the
window over the calls; the median of --reps windows (all of them kept).  Writes one JSON object to
--out and prints it.
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--churn", type=float, default=0.02)
    ap.add_argument("--step-groups", type=int, default=1000)
    ap.add_argument("--step-ids", choices=["random", "mod3", "mod7", "skew"], default="random",
                    help="the step's ids: uniform over the groups; row %% 3; row %% 7; or a half, a quarter and an eighth of "
                         "the rows in groups 0, 1, 2 and the rest uniform")
    ap.add_argument("--step-only", action="store_true", help="the step and the mark only (no read cases)")
    ap.add_argument("--out", default=os.path.join("profiles", "window", "bench.json"))
    args = ap.parse_args()

    import torch

    from kepler_amd import accel, fleet
    from kepler_amd.torch_batch import current_stream_handle, interval_from_tensors, to_device, top_rows_from_tensors

    torch.cuda.set_device(0)
    torch.cuda.set_stream(torch.cuda.Stream())
    s = current_stream_handle()
    L = fleet.config_layout(3, nodes=args.nodes or None)
    Z, N, P = L.zones, L.n_nodes, L.n_procs
    sizes, flag = L.sizes(), L.fast_flag()
    per_node = np.diff(L.proc_off.astype(np.int64))
    slot_off = np.r_[0, np.cumsum(per_node * 5 // 4 + 8)].astype(np.uint32)
    S = int(slot_off[-1])
    caps = L.capacities()
    caps["proc_slots"] = S
    acc = accel.Accel(Z, **caps)
    sm = accel.SlotMap(acc, accel.KACC_KIND_PROC, slot_off)
    sm.set_policy(accel.KACC_JOIN_REUSE_TERMINATED)
    sim = fleet.FleetSim(L, churn=0.0)
    churn = fleet.ProcChurn(L, churn=args.churn)
    n_sets = 4
    keys = [torch.from_numpy(churn.next_keys().view(np.int32)).cuda() for _ in range(args.steps + 2)]
    t = to_device(sim.next_interval())
    t_next = [to_device({k: v for k, v in sim.next_interval().items()
                         if k in ("node_ts_ns", "zone_energy", "node_usage_ratio")}) for _ in range(n_sets)]
    tk = torch.zeros(S, dtype=torch.int64, device="cuda")
    ts = torch.zeros(S, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(N, dtype=torch.int32, device="cuda")
    span = torch.zeros(2 * N, dtype=torch.int32, device="cuda")
    t["node_proc_span"] = span
    rows = top_rows_from_tensors(t, accel.KACC_KIND_PROC)
    rng = np.random.default_rng(1)

    def ids(n_groups):
        return torch.from_numpy(rng.integers(0, n_groups, P).astype(np.uint32).view(np.int32)).cuda()

    tr = accel.Tracker(acc, accel.KACC_KIND_PROC, 500, zone=0, min_energy=10 * 10**6)  # config.go:210-211
    win = accel.Window(acc, accel.KACC_KIND_PROC, args.step_groups)
    if args.step_ids == "random":
        d_ids = ids(args.step_groups)
    else:
        g = rng.integers(0, args.step_groups, P).astype(np.uint32)
        if args.step_ids in ("mod3", "mod7"):
            g = (np.arange(P) % int(args.step_ids[3:])).astype(np.uint32)
        else:
            u = rng.random(P)
            g[u < 0.875] = 2
            g[u < 0.75] = 1
            g[u < 0.5] = 0
        d_ids = torch.from_numpy(g.view(np.int32)).cuda()

    def join(k):
        sm.join(P, t["proc_off"].data_ptr(), keys[k].data_ptr(), 0, t["proc_slot"].data_ptr(), tk.data_ptr(),
                ts.data_ptr(), cnt.data_ptr(), s, span.data_ptr())

    def step():
        win.step(rows, d_ids.data_ptr(), 0, sm, ts.data_ptr(), cnt.data_ptr(), s)

    # the first interval: every ID new
    join(0)
    tr.add(sm, tk.data_ptr(), ts.data_ptr(), cnt.data_ptr(), s)
    step()
    acc.run_interval(interval_from_tensors(t, sizes, flag), s)
    win.mark(s)
    acc.sync(s)
    stage = {"join": [], "tracker_add": [], "window_step": [], "interval": []}
    n_new, n_term = [], []
    for i in range(args.steps):
        t.update(t_next[i % n_sets])
        it = interval_from_tensors(t, sizes, flag)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        e[0].record()
        join(1 + i)
        e[1].record()
        tr.add(sm, tk.data_ptr(), ts.data_ptr(), cnt.data_ptr(), s)
        e[2].record()
        step()
        e[3].record()
        acc.run_interval(it, s)
        e[4].record()
        e[4].synchronize()
        for name, a, b in (("join", 0, 1), ("tracker_add", 1, 2), ("window_step", 2, 3), ("interval", 3, 4)):
            stage[name].append(e[a].elapsed_time(e[b]))
        n_term.append(int(cnt.sum().item()))
        n_new.append(int((t["proc_slot"] < 0).sum().item()))  # KACC_SLOT_NEW is the sign bit of the i32 view
    acc.sync(s)
    med = {k: float(np.median(v)) for k, v in stage.items()}
    new, term = float(np.median(n_new)), float(np.median(n_term))
    step_bytes = 4 * P + new * (8 + 8 * Z) + term * (12 + 16 * Z + 8 * Z + 4)
    step_doc = {
        "policy": "KACC_JOIN_REUSE_TERMINATED, fleet.ProcChurn", "churn": args.churn, "n_groups": args.step_groups,
        "ids": args.step_ids, "merge_rounds_env": os.environ.get("KACC_WINDOW_MERGE_ROUNDS"),
        "steps": args.steps, "median_ms": med, "all_ms": stage, "new_rows_median": new, "terminated_median": term,
        "algorithmic_bytes": step_bytes, "GBps": step_bytes / med["window_step"] / 1e6,
        "frac_of_8TBps_spec": step_bytes / med["window_step"] / 1e6 / HBM_SPEC_GBPS,
        "step_over_interval": med["window_step"] / med["interval"],
        "step_over_join_tracker_interval": med["window_step"] / (med["join"] + med["tracker_add"] + med["interval"]),
        "step_over_tracker_add": med["window_step"] / med["tracker_add"],
    }
    print(json.dumps({"step": step_doc["median_ms"], "share": step_doc["step_over_join_tracker_interval"]}), flush=True)

    def window_ms(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.calls

    # the step without terminated lists: the adopt phase alone, on the last interval's rows
    adopt_all = []
    for _ in range(args.warmup):
        win.step(rows, d_ids.data_ptr(), 0, stream=s)
    for _ in range(args.reps):
        adopt_all.append(window_ms(lambda: win.step(rows, d_ids.data_ptr(), 0, stream=s)))
    step_doc["adopt_only_ms"] = float(np.median(adopt_all))
    step_doc["adopt_only_all_ms"] = adopt_all
    print(json.dumps({"adopt_only_ms": step_doc["adopt_only_ms"]}), flush=True)
    mark_all = []
    for _ in range(args.warmup):
        win.mark(s)
    for _ in range(args.reps):
        mark_all.append(window_ms(lambda: win.mark(s)))
    mark_bytes = 16 * Z * S
    mark_doc = {"ms": float(np.median(mark_all)), "all_ms": mark_all, "slots": S, "algorithmic_bytes": mark_bytes,
                "GBps": mark_bytes / float(np.median(mark_all)) / 1e6}
    win.close()
    tr.close()

    reads = []
    out_row = torch.empty(P * Z, dtype=torch.int64, device="cuda")
    for G in (() if args.step_only else (8, 1000, 10000, 65536)):
        w = accel.Window(acc, accel.KACC_KIND_PROC, G)
        g = ids(G)
        w.step(rows, g.data_ptr(), accel.KACC_WINDOW_ASSIGN_ALL, stream=s)  # attach to the running fleet
        c32 = [torch.empty(G, dtype=torch.int32, device="cuda") for _ in range(4)]
        u64 = [torch.empty(G * Z, dtype=torch.int64, device="cuda") for _ in range(5)]
        p64 = torch.empty(G * Z, dtype=torch.float64, device="cuda")

        def read():
            w.read(rows, 0, c32[0].data_ptr(), u64[0].data_ptr(), u64[1].data_ptr(), c32[1].data_ptr(),
                   u64[2].data_ptr(), out_row.data_ptr(), s)

        def sums():
            acc.group_sums(accel.KACC_KIND_PROC, rows, g.data_ptr(), G, 0, c32[2].data_ptr(), u64[3].data_ptr(),
                           u64[4].data_ptr(), p64.data_ptr(), c32[3].data_ptr(), s)

        for _ in range(args.warmup):
            read()
            sums()
        acc.sync(s)
        r_ms, g_ms = [], []
        for _ in range(args.reps):  # alternated
            g_ms.append(window_ms(sums))
            r_ms.append(window_ms(read))
        acc.sync(s)
        same = bool(torch.equal(c32[0], c32[2]))  # every listed row is in the window
        rb, gb = P * (8 + 24 * Z), P * (8 + 8 * Z + 8)
        rm, gm = float(np.median(r_ms)), float(np.median(g_ms))
        r = {"n_groups": G, "read_ms": rm, "group_sums_ms": gm, "read_all_ms": r_ms, "group_sums_all_ms": g_ms,
             "read_bytes": rb, "group_sums_bytes": gb, "read_GBps": rb / rm / 1e6, "group_sums_GBps": gb / gm / 1e6,
             "read_frac_of_8TBps_spec": rb / rm / 1e6 / HBM_SPEC_GBPS, "time_ratio": rm / gm, "byte_ratio": rb / gb,
             "bins": "LDS, replicated" if G * (1 + Z) < 4096 else "LDS, one copy" if G * (1 + Z) <= 9984
                     else "global atomics",
             "counts_equal_group_sums": same}
        reads.append(r)
        print(json.dumps({k: r[k] for k in ("n_groups", "read_ms", "group_sums_ms", "time_ratio", "byte_ratio")}),
              flush=True)
        w.close()
    acc.close()
    doc = {
        "bench": "tools/bench_window.py", "config": 3, "nodes": N, "processes": P, "process_slots": S, "zones": Z,
        "calls": args.calls, "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
        "method": "step: one HIP event between the stages of join -> tracker add -> window step -> interval, median "
                  "over `steps` intervals; read, group sums, mark: one HIP event pair around `calls` back-to-back "
                  "calls, ms per call = window / calls, median of `reps` windows, read and group sums alternated",
        "bytes": "step: 4 per row + (8 + 8 Z) per NEW row + (16 + 24 Z) per terminated slot; read per row: 8 + 24 Z; "
                 "group sums per row: 16 + 8 Z; mark: 16 Z per slot; accumulators and per-group outputs not counted",
        "step": step_doc, "mark": mark_doc, "read": reads,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": args.out}))


if __name__ == "__main__":
    main()
