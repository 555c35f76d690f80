#!/usr/bin/env python3
"""The terminated half of a scrape at config 3's fleet size (10k nodes, Z = 4) on one MI355X:
kacc_tracker_read (all four outputs) and kacc_format_lines_dev on its result, against what a
caller did before — kacc_tracker_items, the synchronous host read, on the same tracker.

Process trackers with max_size 500, filled by one kacc_tracker_add to a realistic mix: 10 % of
the nodes empty, 75 % partly filled (most of them with few items), 15 % full.  One HIP event
pair around each call; median of --reps repetitions after --warmup.  Before every repetition a
512 MiB buffer is overwritten, so no call finds the tracker's sets or the previous repetition's
outputs in the 256 MiB Infinity Cache.  kacc_tracker_items is given the item count (a caller
without it pays a second, sizing call).  A tool, not a gate: writes one JSON object to --out
and prints it.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_SPEC_GBPS = 8000.0


def fleet_mix(nodes, max_size, rng):
    """Items per node: 10 % empty, 15 % full, the rest 1 .. max_size - 1 with a long tail
    (median about 40)."""
    kind = rng.random(nodes)
    part = np.clip(rng.lognormal(np.log(40.0), 1.0, size=nodes).astype(np.int64), 1, max_size - 1)
    return np.where(kind < 0.10, 0, np.where(kind < 0.25, max_size, part))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10_000)
    ap.add_argument("--max-size", type=int, default=500)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "tracker_export", "bench.json"))
    args = ap.parse_args()

    import torch

    from kepler_amd import accel
    from kepler_amd.torch_batch import current_stream_handle

    torch.cuda.set_device(0)
    torch.cuda.set_stream(torch.cuda.Stream())
    s = current_stream_handle()
    Z, N, K = 4, args.nodes, args.max_size
    rng = np.random.default_rng(3)
    sizes = fleet_mix(N, K, rng)
    slot_off = np.r_[0, np.cumsum(np.maximum(sizes, 1))].astype(np.uint32)
    S = int(slot_off[-1])
    total = int(sizes.sum())
    acc = accel.Accel(Z, nodes=N, proc_slots=S, ctr_slots=1, vm_slots=1, pod_slots=1)
    node_of = np.repeat(np.arange(N), np.diff(slot_off.astype(np.int64)))
    energy = (rng.lognormal(18, 2, size=(S, Z))).astype(np.uint64) + 1
    energy[:, 0] = 10**6 + rng.permutation(S).astype(np.uint64) * 5  # distinct: one order
    acc.upload("proc_energy", energy.reshape(-1))
    acc.upload("proc_ratio", rng.random(S))
    acc.upload("proc_node", node_of.astype(np.uint32))
    acc.upload("node_active_power", rng.random(N * Z) * 1e8 + 1.0)
    acc.upload("node_active_energy", np.ones(N * Z, dtype=np.uint64))
    acc.upload("node_cpu_delta", np.ones(N))
    sm = accel.SlotMap(acc, accel.KACC_KIND_PROC, slot_off)
    tr = accel.Tracker(acc, accel.KACC_KIND_PROC, K, zone=0, min_energy=0)
    tk = torch.from_numpy(100_000 + np.arange(S, dtype=np.int64)).cuda()
    ts = torch.from_numpy(np.arange(S, dtype=np.int32)).cuda()
    tc = torch.from_numpy(sizes.astype(np.int32)).cuda()
    tr.add(sm, tk.data_ptr(), ts.data_ptr(), tc.data_ptr(), s)
    acc.sync(s)

    flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")

    def timed(call):
        ms, wall = [], []
        for rep in range(args.warmup + args.reps):
            flush.fill_(rep)
            torch.cuda.current_stream().synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            if rep >= args.warmup:
                ms.append(e0.elapsed_time(e1))
                wall.append((time.perf_counter() - t0) * 1e3)
        acc.sync(s)
        return float(np.median(ms)), ms, float(np.median(wall))

    # ---- kacc_tracker_read, all four outputs ---------------------------------------
    d_off = torch.zeros(N + 1, dtype=torch.int32, device="cuda")
    tr.read(d_off.data_ptr(), 0, stream=s)  # sizing call
    acc.sync(s)
    assert int(d_off[-1].item()) == total, (int(d_off[-1].item()), total)
    d_key = torch.zeros(total, dtype=torch.int64, device="cuda")
    d_node = torch.zeros(total, dtype=torch.int32, device="cuda")
    d_e = torch.zeros(total * Z, dtype=torch.int64, device="cuda")
    d_p = torch.zeros(total * Z, dtype=torch.float64, device="cuda")
    read_ms, read_all, read_wall = timed(lambda: tr.read(
        d_off.data_ptr(), total, d_key.data_ptr(), d_node.data_ptr(), d_e.data_ptr(), d_p.data_ptr(), stream=s))
    read_bytes = total * (20 + 32 * Z) + (N + 1) * 40  # sets in, outputs out; size -> counts -> scan -> node_off

    # ---- kacc_tracker_items on the same tracker (unchanged; the path before) ------------
    h_key = np.zeros(total, np.uint64)
    h_node = np.zeros(total, np.uint32)
    h_e = np.zeros((total, Z), np.uint64)
    h_p = np.zeros((total, Z), np.float64)
    cnt = ctypes.c_uint32()

    def items_call():
        acc._check(acc.lib.kacc_tracker_items(tr.handle, ctypes.byref(cnt), h_key.ctypes.data, h_node.ctypes.data,
                                              h_e.ctypes.data, h_p.ctypes.data))
    items_ms, items_all, items_wall = timed(items_call)
    same = bool(cnt.value == total and np.array_equal(d_key.cpu().numpy().view(np.uint64), h_key)
                and np.array_equal(d_node.cpu().numpy().view(np.uint32), h_node)
                and np.array_equal(d_e.cpu().numpy().view(np.uint64).reshape(-1, Z), h_e)
                and np.array_equal(d_p.cpu().numpy().view(np.uint64).reshape(-1, Z), h_p.view(np.uint64)))
    items_bytes = total * (12 + 16 * Z)  # what crosses to the host

    # ---- kacc_format_lines_dev on the read's result -------------------------------------
    # fixed-width per-item labels with state="terminated": comm, exe, node_name and pid digits
    head = b'comm="terminated-proc",container_id="",exe="/usr/bin/terminated-proc",node_name="node-'
    tail = b'",state="terminated",type="regular",vm_id=""'
    body = np.frombuffer(head + b"00000" + b'",pid="00000000' + tail, np.uint8)
    L = body.size
    labels = np.tile(body, (total, 1))
    keys = d_key.cpu().numpy().view(np.uint64)
    nodes_h = d_node.cpu().numpy().view(np.uint32).astype(np.int64)
    labels[:, len(head):len(head) + 5] = np.array([(nodes_h // 10 ** k) % 10 for k in range(4, -1, -1)],
                                                  dtype=np.uint8).T + ord("0")
    p0 = len(head) + 5 + len(b'",pid="')
    labels[:, p0:p0 + 8] = np.array([(keys // np.uint64(10 ** k)) % np.uint64(10) for k in range(7, -1, -1)],
                                    dtype=np.uint8).T + ord("0")
    d_labels = torch.from_numpy(labels.reshape(-1)).cuda()
    d_loff = torch.from_numpy(np.arange(total + 1, dtype=np.int64) * L).cuda()
    zone_names = ["package", "core", "uncore", "dram"]
    lines = total * Z
    d_line_off = torch.zeros(lines + 1, dtype=torch.int64, device="cuda")
    fmt = {}
    for what, is_energy, src, metric in (("joules", True, d_e, "kepler_process_cpu_joules_total"),
                                         ("watts", False, d_p, "kepler_process_cpu_watts")):
        a = (is_energy, src.data_ptr(), total, metric, zone_names, d_labels.data_ptr(), d_loff.data_ptr(),
             d_line_off.data_ptr())
        text = acc.format_lines_dev(*a, stream=s)
        out = torch.empty(text, dtype=torch.uint8, device="cuda")
        ms, all_ms, wall = timed(lambda: acc.format_lines_dev(*a, out_ptr=out.data_ptr(), out_cap=text, stream=s))
        nbytes = text + total * L + 16 * lines + 8 * total  # text out; labels, values (two passes), offsets
        fmt[what] = {"ms": ms, "all_ms": all_ms, "host_wall_ms": wall, "text_bytes": text, "lines": lines,
                     "algorithmic_bytes": nbytes, "GBps": nbytes / ms / 1e6,
                     "frac_of_8TBps_spec": nbytes / ms / 1e6 / HBM_SPEC_GBPS}
        del out
    acc.close()

    doc = {
        "bench": "tools/bench_tracker_export.py", "device": torch.cuda.get_device_name(0),
        "nodes": N, "zones": Z, "max_size": K, "items": total,
        "node_mix": {"empty": int((sizes == 0).sum()), "partly": int(((sizes > 0) & (sizes < K)).sum()),
                     "full": int((sizes == K).sum()), "median_partly": float(np.median(sizes[(sizes > 0) & (sizes < K)]))},
        "reps": args.reps, "warmup": args.warmup,
        "method": "one HIP event pair around the call; median; a 512 MiB buffer overwritten before every repetition",
        "tracker_read": {"ms": read_ms, "all_ms": read_all, "host_wall_ms": read_wall, "bytes": read_bytes,
                         "GBps": read_bytes / read_ms / 1e6,
                         "frac_of_8TBps_spec": read_bytes / read_ms / 1e6 / HBM_SPEC_GBPS},
        "tracker_items": {"ms": items_ms, "all_ms": items_all, "host_wall_ms": items_wall,
                          "bytes_to_host": items_bytes, "GBps_to_host": items_bytes / items_ms / 1e6},
        "read_equals_items": same,
        "items_over_read": items_ms / read_ms if read_ms > 0 else None,
        "read_faster_than_items": read_ms < items_ms,
        "format_lines_dev": fmt,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
