// The node kernels' shared rules (device helpers of kacc_engine.hip, not part of
// the public ABI).  interval_node (interval_kernel, interval_sums_kernel), intervals_carry_kernel,
// small_kernel and chunk_kernel (+ big_node_prepare, pod_kernel) compute the same node snapshot
// with different shapes of workgroup.  What they share is here, once:
//   * the device state, the error bits, block-uniform values, the row loads and stores, one
//     row's attribution (process.go:118-148 and its container / VM / pod twins), the exports;
//   * a node's row ranges and their clamp;
//   * the per-node rules of the reference that every kernel restates: which aggregate a lane
//     holds and where its segment begins and ends, the clamp of a malformed segment, a
//     container's / VM's / pod's CPU time, the node scalars of the new snapshot, the slot-sweep
//     decision and its inverse map, a 64-row group's previous totals, the per-role tables, the
//     256-leaf node-total tree on 64 lanes, and an aggregate's outputs.
// Every helper is a plain function over the caller's registers and LDS arrays: nothing here
// holds a value across a barrier, so a kernel that re-derives a role or a table pointer at each
// use (interval_node does, to keep VGPRs dead) still does.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/kepler_accel.h"
#include "kacc_device.hpp"

namespace kacc {

constexpr int kTree = 256;  // lanes of the canonical node-total tree

// device error bits (KACC_ERANGE)
constexpr uint32_t kErrNode = 1u << 0;
constexpr uint32_t kErrOffsets = 1u << 1;
constexpr uint32_t kErrSlot = 1u << 2;
constexpr uint32_t kErrNs = 1u << 3;
constexpr uint32_t kErrCapacity = 1u << 4;
constexpr uint32_t kErrBigNode = 1u << 5;  // oversized node under KACC_F_FAST_NODES

// One big-node chunk (see big_node_prepare).  ctr_begin / vm_begin / pod_begin:
// the first container / VM / pod the chunk owns; it owns them up to the next
// chunk's begin (or the node's end for the last chunk).
struct ChunkItem {
  uint32_t node, chunk, nchunks, ctr_begin, vm_begin, pod_begin, pad[2];
};

struct DevState {
  uint64_t *node_energy_total, *node_active_energy, *node_active_total, *node_idle_total;
  double *node_power, *node_active_power, *node_idle_power;
  int64_t *node_ts;
  uint32_t *node_has_prev;
  double *node_usage_ratio, *node_cpu_delta;
  uint32_t *node_status;
  uint64_t *proc_energy;
  double *proc_ratio;   // [Sp] cpuTimeRatio of the slot's last attribution (power is derived)
  uint32_t *proc_node;  // [Sp] the node that attribution belonged to
  uint64_t *ctr_energy;
  double *ctr_ratio, *ctr_cpu_delta, *ctr_cpu_total;  // container / VM power is derived (as processes')
  uint32_t *ctr_node;
  uint64_t *vm_energy;
  double *vm_ratio, *vm_cpu_delta;
  uint32_t *vm_node;
  uint64_t *pod_energy;
  double *pod_power, *pod_cpu_delta, *pod_cpu_total;
  uint64_t proc_slots, ctr_slots, vm_slots, pod_slots;
  uint32_t *err;
  uint2 *defer;        // [defer_cap] (node, pod) pods left to pod_kernel
  uint32_t *defer_ctr;  // [0] length; re-armed by interval_kernel
  uint32_t defer_cap;
  ChunkItem *items;    // [item_cap] big-node chunks this launch
  uint32_t *item_ctr;  // [0] length, [1] dequeue head; cleared by pod_kernel
  uint32_t item_cap;
  // kacc_run_intervals over intervals of ONE layout (the same offset arrays):
  // the chunk items are generated once (items_kernel) and reused, so the node
  // phase skips them; pod_kernel keeps the list for the next interval
  uint32_t items_given, keep_items;
  uint64_t *stamps;  // kVarStamps only
};

struct NodeShared {
  uint64_t active_energy[KACC_MAX_ZONES];
  double power[KACC_MAX_ZONES];
  double active_power[KACC_MAX_ZONES];
  double node_delta;
  uint32_t first;
};

__device__ __forceinline__ void raise_err(uint32_t *err, uint32_t bit) { atomicOr(err, bit); }

// Block-uniform values live in SGPRs (saves VGPRs for rows in flight).
__device__ __forceinline__ uint64_t uniform_u64(uint64_t x) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(x));
  const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(x >> 32));
  return (static_cast<uint64_t>(hi) << 32) | lo;
}
__device__ __forceinline__ double uniform_f64(double x) {
  return __longlong_as_double(static_cast<long long>(uniform_u64(static_cast<uint64_t>(__double_as_longlong(x)))));
}
__device__ __forceinline__ uint32_t uniform_u32(uint32_t x) { return __builtin_amdgcn_readfirstlane(x); }
// a table pointer held in SGPRs, still known to be global memory (a pointer rebuilt from
// an integer is generic: flat loads, which count on lgkmcnt too)
template <typename T>
__device__ __forceinline__ const T __attribute__((address_space(1))) *uniform_ptr(const T *p) {
  return (const T __attribute__((address_space(1))) *)uniform_u64(reinterpret_cast<uint64_t>(p));
}

// Experiments (timing A/B only; results are identical): KACC_WT_PROC writes the
// non-temporal row stores through the L2 (sc0 sc1 nt: no dirty line is left for
// the end-of-kernel write-back), KACC_WT_AGG the aggregate rows likewise.
// Experiment: extra dynamic LDS per interval_kernel workgroup (fewer resident
// workgroups per CU, each with a larger share of the bandwidth: shorter lifetimes)
#ifndef KACC_FAST_EXTRA_LDS
#define KACC_FAST_EXTRA_LDS 0
#endif
#ifndef KACC_WT_PROC
#define KACC_WT_PROC 0
#endif
#ifndef KACC_WT_AGG
#define KACC_WT_AGG 0
#endif
template <typename T>
__device__ __forceinline__ void wt_store(T v, T *p) {
  if constexpr (sizeof(T) == 16)
    asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1 nt" ::"v"(p), "v"(v) : "memory");
  else if constexpr (sizeof(T) == 8)
    asm volatile("global_store_dwordx2 %0, %1, off sc0 sc1 nt" ::"v"(p), "v"(v) : "memory");
  else
    asm volatile("global_store_dword %0, %1, off sc0 sc1 nt" ::"v"(p), "v"(v) : "memory");
}
template <typename T>
__device__ __forceinline__ void nt_store(T v, T *p) {
  if constexpr (KACC_WT_PROC != 0)
    wt_store(v, p);
  else
    __builtin_nontemporal_store(v, p);
}

template <int Z>
__device__ __forceinline__ void load_row(const uint64_t *__restrict__ base, uint64_t s,
                                         uint64_t (&out)[Z]) {
  if constexpr (Z % 2 == 0) {
    using u64x2 = __attribute__((ext_vector_type(2))) unsigned long long;
    const u64x2 *p = reinterpret_cast<const u64x2 *>(base + s * Z);
#pragma unroll
    for (int k = 0; k < Z / 2; ++k) {
      const u64x2 x = p[k];
      out[2 * k] = x.x;
      out[2 * k + 1] = x.y;
    }
  } else {
#pragma unroll
    for (int z = 0; z < Z; ++z) out[z] = base[s * Z + z];
  }
}

template <int Z>
__device__ __forceinline__ void load_row_f64(const double *__restrict__ base, uint64_t s,
                                             double (&out)[Z]) {
  if constexpr (Z % 2 == 0) {
    using f64x2 = __attribute__((ext_vector_type(2))) double;
    const f64x2 *p = reinterpret_cast<const f64x2 *>(base + s * Z);
#pragma unroll
    for (int k = 0; k < Z / 2; ++k) {
      const f64x2 x = p[k];
      out[2 * k] = x.x;
      out[2 * k + 1] = x.y;
    }
  } else {
#pragma unroll
    for (int z = 0; z < Z; ++z) out[z] = base[s * Z + z];
  }
}

template <int Z, bool NT, typename T>
__device__ __forceinline__ void store_row(T *__restrict__ base, uint64_t s, const T (&in)[Z]) {
  if constexpr (Z % 2 == 0) {
    using v2 = __attribute__((ext_vector_type(2))) T;
    v2 *p = reinterpret_cast<v2 *>(base + s * Z);
#pragma unroll
    for (int k = 0; k < Z / 2; ++k) {
      v2 x;
      x.x = in[2 * k];
      x.y = in[2 * k + 1];
      if constexpr (NT)
        nt_store(x, p + k);
      else
        p[k] = x;
    }
  } else {
#pragma unroll
    for (int z = 0; z < Z; ++z) {
      if constexpr (NT)
        nt_store(in[z], base + s * Z + z);
      else
        base[s * Z + z] = in[z];
    }
  }
}

// Pod rows are stored as one record per slot: the Z energy words then the Z
// power words (KACC_T_POD_POWER's base is KACC_T_POD_ENERGY's + Z words), so a
// pod's row is ONE 64-B gather at Z = 4 for the namespace totals (two 32-B rows
// of two tables before: cluster partials 31.5 -> 22.0 us at config 3,
// profiles/r03/abns).  load_row / store_row address base + s*Z, so a pod slot s
// is passed as row 2s.
constexpr uint64_t kPodRowScale = 2;
__device__ __forceinline__ uint64_t pod_row(uint64_t s) { return s * kPodRowScale; }
// the row index of aggregate slot s in its role's tables (1 container, 2 VM, 3 pod)
__device__ __forceinline__ uint64_t agg_row(uint32_t role, uint64_t s) { return role == 3 ? pod_row(s) : s; }

// Node-uniform attribution parameters (SGPRs) for the row passes.
template <int Z>
struct Attr {
  uint64_t aE[Z];  // NodeUsage.activeEnergy
  double aP[Z];    // NodeUsage.ActivePower
  uint32_t live;   // bit z: zone passes the guard (ActivePower, activeEnergy, ΔcpuNode)
  uint32_t live_pod;  // pod.go:96 guards on Power instead of ActivePower
  double nd;       // ProcessTotalCPUTimeDelta
  uint32_t first;  // first*Read variant: EnergyTotal = interval energy, Power 0
  // KACC_F_STABLE_SLOT_NODES on a node past its first read: a row's slot already
  // holds this node in KACC_T_PROC_NODE unless the row is NEW, so only NEW rows
  // store it (4 B per process row less HBM traffic)
  uint32_t keep_node;
};

// Attr from the node phase's LDS results (block-uniform -> SGPRs).
template <int Z>
__device__ __forceinline__ Attr<Z> make_attr(const NodeShared &sh, uint32_t flags) {
  Attr<Z> a;
  a.nd = uniform_f64(sh.node_delta);
  a.first = uniform_u32(sh.first);
  a.keep_node = (flags & KACC_F_STABLE_SLOT_NODES) && !a.first ? 1u : 0u;
  a.live = 0;
  a.live_pod = 0;
#pragma unroll
  for (int z = 0; z < Z; ++z) {
    a.aE[z] = uniform_u64(sh.active_energy[z]);
    a.aP[z] = uniform_f64(sh.active_power[z]);
    const double pw = uniform_f64(sh.power[z]);
    const bool ok = a.aE[z] != 0 && a.nd != 0;
    if (ok && a.aP[z] != 0) a.live |= 1u << z;                       // process.go:124
    if (ok && (a.first ? a.aP[z] : pw) != 0) a.live_pod |= 1u << z;  // pod.go:96 / :23
  }
  return a;
}

// process.go:118-148 (and its container/VM/pod twins) for one row.
template <int Z>
__device__ __forceinline__ double attribute_row(const Attr<Z> &a, uint32_t live, double delta,
                                                bool is_new, const uint64_t (&prev)[Z],
                                                uint64_t (&E)[Z], double (&P)[Z]) {
  const double ratio = delta / a.nd;  // one IEEE division per row, never a reciprocal
#pragma unroll
  for (int z = 0; z < Z; ++z) {
    if (live & (1u << z)) {
      const uint64_t e = go_f64_to_u64(ratio * u2f(a.aE[z]));
      E[z] = a.first ? e : e + (is_new ? 0ull : prev[z]);
      P[z] = a.first ? 0.0 : ratio * a.aP[z];
    } else {  // skipped zone keeps the zero Usage of newProcess (process.go:58-63)
      E[z] = 0;
      P[z] = 0.0;
    }
  }
  return ratio;
}

// process.go:118-148 for one process row: the energy totals, and the row's
// cpuTimeRatio (returned), which the state keeps INSTEAD of the Z powers: a
// process's Power is ratio · the node's ActivePower when the zone passes the
// guard (process.go:124, 142) — a function of the node's own tables of the same
// interval (kacc_derive.hpp), derived wherever it is read.  8 + 4 bytes per row
// (ratio, node) instead of 8Z.
template <int Z>
__device__ __forceinline__ double attribute_proc(const Attr<Z> &a, double delta, bool is_new,
                                                 const uint64_t (&prev)[Z], uint64_t (&E)[Z]) {
  const double ratio = delta / a.nd;  // one IEEE division per row, never a reciprocal
#pragma unroll
  for (int z = 0; z < Z; ++z) {
    if (a.live & (1u << z)) {
      const uint64_t e = go_f64_to_u64(ratio * u2f(a.aE[z]));
      E[z] = a.first ? e : e + (is_new ? 0ull : prev[z]);
    } else {  // skipped zone keeps the zero Usage of newProcess (process.go:58-63)
      E[z] = 0;
    }
  }
  return ratio;
}

// A process row's outputs at slot s: energy totals, ratio and node.
template <int Z, bool NT>
__device__ __forceinline__ void store_proc(const DevState &st, uint64_t s, const uint64_t (&E)[Z], double ratio,
                                           uint32_t node, bool wnode) {
  store_row<Z, NT, uint64_t>(st.proc_energy, s, E);
  if constexpr (NT) {
    nt_store(ratio, st.proc_ratio + s);
    if (wnode) nt_store(node, st.proc_node + s);
  } else {
    st.proc_ratio[s] = ratio;
    if (wnode) st.proc_node[s] = node;
  }
}

// Cluster-total exports (kacc_interval.pod_export / node_export): what a pod /
// node contributes to the cluster totals, in batch order, written by the
// interval's own kernels so that kacc_allreduce_exports reduces them on
// another stream while the next interval runs.  Pod row q: EnergyTotal[Z] then
// the bits of Power[Z] (zeros for a pod whose slot is out of range).
// Plain stores: a lane's record leaves as Z/2 + Z/2 16-B pieces, so each wave
// instruction writes every 2Z-th 16 B of the wave's span; L2 merges the pieces
// into full lines (non-temporal, each piece would reach HBM as a partial line).
// The export row of batch pod q (kacc_interval.pod_export_pos: namespace order),
// or ~0u when it is out of range (raised; nothing is written).
__device__ __forceinline__ uint32_t export_row(const kacc_interval &b, uint32_t q, uint32_t *err) {
  if (!b.pod_export_pos) return q;
  const uint32_t r = b.pod_export_pos[q];
  if (r >= b.n_pods) {
    atomicOr(err, 1u << 1);  // kErrOffsets
    return ~0u;
  }
  return r;
}
template <int Z>
__device__ __forceinline__ void export_pod_at(const kacc_interval &b, uint32_t row, const uint64_t (&E)[Z],
                                              const double (&P)[Z]) {
  if (!b.pod_export || row == ~0u) return;
  uint64_t *o = b.pod_export + static_cast<uint64_t>(row) * (2 * Z);
  store_row<Z, false, uint64_t>(o, 0, E);
  store_row<Z, false, double>(reinterpret_cast<double *>(o), 1, P);
}
template <int Z>
__device__ __forceinline__ void export_pod(const kacc_interval &b, uint32_t q, const uint64_t (&E)[Z],
                                           const double (&P)[Z], uint32_t *err) {
  if (!b.pod_export) return;
  export_pod_at<Z>(b, export_row(b, q, err), E, P);
}
template <int Z>
__device__ __forceinline__ void export_pod_zero(const kacc_interval &b, uint32_t q, uint32_t *err) {
  uint64_t E[Z];
  double P[Z];
#pragma unroll
  for (int z = 0; z < Z; ++z) {
    E[z] = 0;
    P[z] = 0.0;
  }
  export_pod<Z>(b, q, E, P, err);
}
// Node n, zone z: ActiveEnergyTotal, IdleEnergyTotal, Power, ActivePower, IdlePower.
template <int Z>
__device__ __forceinline__ void export_node_zone(const kacc_interval &b, uint32_t n, uint32_t z, uint64_t at,
                                                 uint64_t it, double p, double ap, double ip) {
  if (!b.node_export) return;
  uint64_t *o = b.node_export + static_cast<uint64_t>(n) * (5 * Z) + z;
  o[0] = at;
  o[Z] = it;
  o[2 * Z] = static_cast<uint64_t>(__double_as_longlong(p));
  o[3 * Z] = static_cast<uint64_t>(__double_as_longlong(ap));
  o[4 * Z] = static_cast<uint64_t>(__double_as_longlong(ip));
}

// An aggregate row's outputs at slot s: energy totals; for a pod its powers,
// for a container / VM its ratio and node (their power is derived on read as
// a process's: the same guard, container.go:106-140, vm.go:78-109).
template <int Z, typename T>
__device__ __forceinline__ void wt_row(T *__restrict__ base, uint64_t s, const T (&in)[Z]) {
  if constexpr (Z % 2 == 0) {
    using v2 = __attribute__((ext_vector_type(2))) T;
    v2 *p = reinterpret_cast<v2 *>(base + s * Z);
#pragma unroll
    for (int k = 0; k < Z / 2; ++k) {
      v2 x;
      x.x = in[2 * k];
      x.y = in[2 * k + 1];
      wt_store(x, p + k);
    }
  } else {
#pragma unroll
    for (int z = 0; z < Z; ++z) wt_store(in[z], base + s * Z + z);
  }
}

template <int Z, bool NT>
__device__ __forceinline__ void store_agg(const DevState &st, uint32_t role, uint64_t s, const uint64_t (&E)[Z],
                                          const double (&P)[Z], double ratio, uint32_t node) {
  if constexpr (KACC_WT_AGG != 0 && !NT) {
    if (role == 3) {
      wt_row<Z, uint64_t>(st.pod_energy, pod_row(s), E);
      wt_row<Z, double>(st.pod_power, pod_row(s), P);
      return;
    }
    wt_row<Z, uint64_t>(role == 1 ? st.ctr_energy : st.vm_energy, s, E);
    wt_store(ratio, (role == 1 ? st.ctr_ratio : st.vm_ratio) + s);
    wt_store(node, (role == 1 ? st.ctr_node : st.vm_node) + s);
    return;
  }
  if (role == 3) {
    store_row<Z, NT, uint64_t>(st.pod_energy, pod_row(s), E);
    store_row<Z, NT, double>(st.pod_power, pod_row(s), P);
    return;
  }
  store_row<Z, NT, uint64_t>(role == 1 ? st.ctr_energy : st.vm_energy, s, E);
  double *r = role == 1 ? st.ctr_ratio : st.vm_ratio;
  uint32_t *nd = role == 1 ? st.ctr_node : st.vm_node;
  if constexpr (NT) {
    nt_store(ratio, r + s);
    nt_store(node, nd + s);
  } else {
    r[s] = ratio;
    nd[s] = node;
  }
}

// A container's CPU time (informer.go:229-233, 481-486): delta and total summed
// over rows [i, e) of s_d in listing order — Go's order, so one lane adds them
// one after the other.  kB reads are issued together per step; a tail step adds
// +0.0 for rows past e, an identity on sums that start at +0.0 (neither sum can
// ever be -0.0), and reads a clamped in-bounds row.
template <int kB>
__device__ __forceinline__ void segment_load(const double *s_d, uint32_t i, uint32_t e, double (&v)[kB]) {
#pragma unroll
  for (int u = 0; u < kB; ++u) v[u] = s_d[min(i + u, e - 1)];  // e > i: in bounds
}
template <int kB>
__device__ __forceinline__ void segment_add(const double (&v)[kB], uint32_t i, uint32_t e, double &delta,
                                            double &total) {
#pragma unroll
  for (int u = 0; u < kB; ++u) {
    const double x = i + u < e ? v[u] : 0.0;
    delta = delta + x;
    total = total + x;
  }
}
// One batch at a time (kernels short of registers).
template <int kB>
__device__ __forceinline__ void segment_sum(const double *s_d, uint32_t i, uint32_t e, double &delta,
                                            double &total) {
  for (; i < e; i += kB) {
    double v[kB];
    segment_load<kB>(s_d, i, e, v);
    segment_add<kB>(v, i, e, delta, total);
  }
}

struct NodeRanges {
  uint32_t p0, p1, c0, c1, v0, v1, q0, q1;
};

// Status and row ranges of node n as ONE batch of vector loads through an index
// the compiler must treat as per-lane, waited for once, then made uniform: as
// scalar loads they took two dependent round trips (the offsets behind the
// status branch) before a workgroup could issue its row loads.
__device__ __forceinline__ void node_words(const kacc_interval &b, uint32_t n, uint32_t &status, NodeRanges &r) {
  uint32_t ni = n;
  asm volatile("" : "+v"(ni));
  const uint32_t *sp = b.node_status ? b.node_status : b.proc_off;  // a stand-in address: no branch
  const uint32_t s = sp[ni];
  uint32_t w[8] = {b.proc_off[ni], b.proc_off[ni + 1], b.ctr_off[ni], b.ctr_off[ni + 1],
                   b.vm_off[ni],   b.vm_off[ni + 1],   b.pod_off[ni], b.pod_off[ni + 1]};
  asm volatile("" ::"v"(s), "v"(w[0]), "v"(w[1]), "v"(w[2]), "v"(w[3]), "v"(w[4]), "v"(w[5]), "v"(w[6]),
               "v"(w[7]));  // the one wait
  status = b.node_status ? __builtin_amdgcn_readfirstlane(s) : 0u;
  auto u = [](uint32_t x) { return static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(x)); };
  r = NodeRanges{u(w[0]), u(w[1]), u(w[2]), u(w[3]), u(w[4]), u(w[5]), u(w[6]), u(w[7])};
}

// Row ranges of node n, clamped so a malformed batch cannot fault.
__device__ __forceinline__ NodeRanges clamp_ranges(const kacc_interval &b, const DevState &st, NodeRanges r,
                                                   int tid) {
  if (r.p1 > b.n_procs || r.p0 > r.p1 || r.c1 > b.n_ctrs || r.c0 > r.c1 || r.v1 > b.n_vms ||
      r.v0 > r.v1 || r.q1 > b.n_pods || r.q0 > r.q1) {
    if (tid == 0) raise_err(st.err, kErrOffsets);
    r.p1 = min(r.p1, b.n_procs);
    r.p0 = min(r.p0, r.p1);
    r.c1 = min(r.c1, b.n_ctrs);
    r.c0 = min(r.c0, r.c1);
    r.v1 = min(r.v1, b.n_vms);
    r.v0 = min(r.v0, r.v1);
    r.q1 = min(r.q1, b.n_pods);
    r.q0 = min(r.q0, r.q1);
  }
  return r;
}
__device__ __forceinline__ NodeRanges node_ranges(const kacc_interval &b, const DevState &st,
                                                  uint32_t n, int tid) {
  return clamp_ranges(b, st,
                      NodeRanges{b.proc_off[n], b.proc_off[n + 1], b.ctr_off[n], b.ctr_off[n + 1], b.vm_off[n],
                                 b.vm_off[n + 1], b.pod_off[n], b.pod_off[n + 1]},
                      tid);
}
// ======================= the per-node rules of the reference ==========================

// ---- which aggregate a lane holds ---------------------------------------------------------
// A node's aggregates in lane order: its nc containers, then its nv VMs, then its nq pods.
// Role of aggregate i: 1 container, 2 VM, 3 pod, 0 none.
__device__ __forceinline__ uint32_t agg_role(uint32_t i, uint32_t nc, uint32_t nv, uint32_t nq) {
  return i < nc ? 1u : i < nc + nv ? 2u : i < nc + nv + nq ? 3u : 0u;
}
// Its position inside the role's range.
__device__ __forceinline__ uint32_t agg_index(uint32_t i, uint32_t nc, uint32_t nv) {
  return i < nc ? i : i < nc + nv ? i - nc : i - nc - nv;
}
// Where aggregate j of a role begins: at the end of the one listed before it (prev_end, read
// only when j > 0).  The first of each role has none; the two quirks of the listing order
// (informer.go:223-326): VM 0 begins at the node's last container end (ctr_rows_end, read only
// when the node has containers), and pod 0 begins at c0.
__device__ __forceinline__ uint32_t agg_begin(const NodeRanges &rg, uint32_t role, uint32_t j, uint32_t prev_end,
                                              uint32_t ctr_rows_end) {
  if (j != 0) return prev_end;
  return role == 1 ? rg.p0 : role == 2 ? (rg.c1 > rg.c0 ? ctr_rows_end : rg.p0) : rg.c0;
}
// Aggregate j of a role (1, 2, 3) of the node: its segment [beg, end) — process rows for a
// container or a VM, containers for a pod, both in batch indices and unclamped (clamp_segment)
// — and its slot word.  Every index read lies inside the node's (clamped) ranges.
__device__ __forceinline__ void agg_segment(const kacc_interval &b, const NodeRanges &rg, uint32_t role, uint32_t j,
                                            uint32_t &beg, uint32_t &end, uint32_t &word) {
  if (role == 1) {
    const uint32_t c = rg.c0 + j;
    beg = agg_begin(rg, 1u, j, j ? b.ctr_proc_end[c - 1] : 0u, 0u);
    end = b.ctr_proc_end[c];
    word = b.ctr_slot[c];
  } else if (role == 2) {
    const uint32_t v = rg.v0 + j;
    beg = agg_begin(rg, 2u, j, j ? b.vm_proc_end[v - 1] : 0u, !j && rg.c1 > rg.c0 ? b.ctr_proc_end[rg.c1 - 1] : 0u);
    end = b.vm_proc_end[v];
    word = b.vm_slot[v];
  } else if (role == 3) {
    const uint32_t q = rg.q0 + j;
    beg = agg_begin(rg, 3u, j, j ? b.pod_ctr_end[q - 1] : 0u, 0u);
    end = b.pod_ctr_end[q];
    word = b.pod_slot[q];
  }
}

// ---- a malformed segment ---------------------------------------------------------------------
// [beg, end) must lie inside [lo, hi] (the node's rows for a container or a VM, its containers
// for a pod) with beg <= end.  One that does not is reported and clamped, so that a bad batch
// cannot fault; kacc_validate_host rejects exactly these batches.
__device__ __forceinline__ void clamp_segment(uint32_t &beg, uint32_t &end, uint32_t lo, uint32_t hi, uint32_t *err) {
  if (beg < lo || end < beg || end > hi) {
    raise_err(err, kErrOffsets);
    beg = max(min(beg, hi), lo);
    end = max(min(end, hi), beg);
  }
}

// ---- CPU time of a container, a VM, a pod ------------------------------------------------------
// Rows [i, e) of s_d (the node's staged Δ).  A container sums them in listing order (segment_sum,
// kB reads in flight); a VM takes the last one: updateVMCache (informer.go:445), the last process
// in listing order wins.
template <int kB>
__device__ __forceinline__ void segment_cpu(const double *s_d, uint32_t role, uint32_t i, uint32_t e, double &delta,
                                            double &total) {
  if (role == 1)
    segment_sum<kB>(s_d, i, e, delta, total);  // resetCPUTime on the first process (informer.go:229-233, 481-486)
  else
    delta = e > i ? s_d[e - 1] : 0.0;
}
// A pod over its containers [first, last) of s_cd / s_ct (informer.go:305-309, 502-507), in order.
__device__ __forceinline__ void pod_sum(const double *s_cd, const double *s_ct, uint32_t first, uint32_t last,
                                        double &delta, double &total) {
  for (uint32_t c = first; c < last; ++c) {
    delta = delta + s_cd[c];
    total = total + s_ct[c];  // quirk: the container's running total
  }
}

// ---- the per-role tables -----------------------------------------------------------------------
__device__ __forceinline__ uint64_t agg_cap(const DevState &st, uint32_t role) {
  return role == 1 ? st.ctr_slots : role == 2 ? st.vm_slots : role == 3 ? st.pod_slots : 0;
}
__device__ __forceinline__ uint64_t *agg_energy(const DevState &st, uint32_t role) {
  return role == 1 ? st.ctr_energy : role == 2 ? st.vm_energy : st.pod_energy;
}
__device__ __forceinline__ double *agg_cpu_total(const DevState &st, uint32_t role) {  // a VM keeps none
  return role == 1 ? st.ctr_cpu_total : st.pod_cpu_total;
}
// An aggregate's CPU time of this interval at its slot s (branches, not a selected table
// pointer: a pointer chosen per lane is two VGPRs and a vector load of the kernel argument).
__device__ __forceinline__ void store_agg_cpu(const DevState &st, uint32_t role, uint64_t s, double delta,
                                              double total) {
  if (role == 1) {
    st.ctr_cpu_delta[s] = delta;
    st.ctr_cpu_total[s] = total;
  } else if (role == 2) {
    st.vm_cpu_delta[s] = delta;
  } else {
    st.pod_cpu_delta[s] = delta;
    st.pod_cpu_total[s] = total;
  }
}
// An aggregate's previous totals and running CPU total (0 for a NEW slot, and for a VM) when its
// slot is inside the table (ok); zeros and kErrSlot otherwise.
template <int Z>
__device__ __forceinline__ void load_agg_prev(const DevState &st, uint32_t role, uint32_t word, bool ok,
                                              uint64_t (&prev)[Z], double &total) {
  const uint32_t s = word & KACC_SLOT_MASK;
  total = 0.0;
  if (ok) {
    load_row<Z>(agg_energy(st, role), agg_row(role, s), prev);
    if (role != 2 && !(word & KACC_SLOT_NEW)) total = agg_cpu_total(st, role)[s];
  } else {
#pragma unroll
    for (int z = 0; z < Z; ++z) prev[z] = 0;
  }
  if (role != 0 && !ok) raise_err(st.err, kErrSlot);
}

// ---- the node scalars of the new snapshot ------------------------------------------------------
// One lane per node, after the node's attribution parameters are known.
__device__ __forceinline__ void store_node_scalars(const DevState &st, uint32_t n, bool first, double node_delta,
                                                   int64_t ts, double usage_ratio) {
  st.node_ts[n] = ts;
  st.node_has_prev[n] = 1u;
  st.node_usage_ratio[n] = first ? 0.0 : usage_ratio;  // firstNodeRead leaves 0
  st.node_cpu_delta[n] = node_delta;
  st.node_status[n] = first ? KACC_NODE_FIRST_READ : KACC_NODE_OK;
}

// ---- the slot sweep ------------------------------------------------------------------------------
// A node's rows are attributed in slot order when its slot span [lo, hi] (kacc_slot_join's
// out_span) fits the kernel's inverse map of `limit` entries and the table.
__device__ __forceinline__ bool span_sweeps(const DevState &st, uint32_t rows, uint32_t lo, uint32_t hi,
                                            uint32_t limit) {
  return rows > 0 && hi >= lo && hi - lo < limit && hi < st.proc_slots;
}
// The same from the batch (node-uniform -> SGPRs): smin and span are set whenever a span is given.
__device__ __forceinline__ bool sweep_span(const kacc_interval &b, const DevState &st, uint32_t n, uint32_t rows,
                                           uint32_t limit, uint32_t &smin, uint32_t &span) {
  if (!b.node_proc_span) return false;
  const uint32_t lo = uniform_u32(b.node_proc_span[2 * n]);
  const uint32_t hi = uniform_u32(b.node_proc_span[2 * n + 1]);
  smin = lo;
  span = hi - lo + 1;
  return span_sweeps(st, rows, lo, hi, limit);
}
// One row's entry of the inverse map (slot - smin -> entry).  A row whose slot lies outside the
// node's span or the table is reported and not attributed.
__device__ __forceinline__ void fill_inverse(const DevState &st, uint16_t *s_inv, uint32_t word, uint32_t smin,
                                             uint32_t span, uint32_t entry) {
  const uint32_t sl = word & KACC_SLOT_MASK;
  if (sl - smin < span && sl < st.proc_slots)
    s_inv[sl - smin] = static_cast<uint16_t>(entry);
  else
    raise_err(st.err, kErrSlot);
}

// ---- a 64-row group's previous totals ------------------------------------------------------------
// This wave's 64 rows (in: the lane's row exists; sl: its slot) hold the 64 consecutive slots
// [g0, g0 + 64) inside the table: the group moves as whole 1 KiB wave instructions
// (load_group_masked / attribute_group_masked).  Wave-uniform.
__device__ __forceinline__ bool group_is_contiguous(const DevState &st, bool in, uint64_t sl, uint64_t &g0) {
  g0 = uniform_u32(static_cast<uint32_t>(sl));  // lane 0's slot
  return __all(in && sl == g0 + (threadIdx.x & 63u) && g0 + 64 <= st.proc_slots);
}
// The per-row fallback: the slot's previous totals, or zeros for no row / a slot past the table
// (reported where the row is attributed).
template <int Z>
__device__ __forceinline__ void load_prev_or_zero(const DevState &st, bool in, uint64_t sl, uint64_t (&prev)[Z]) {
  if (in && sl < st.proc_slots) {
    load_row<Z>(st.proc_energy, sl, prev);
  } else {
#pragma unroll
    for (int z = 0; z < Z; ++z) prev[z] = 0;
  }
}

// ---- ProcessTotalCPUTimeDelta (informer.go:330-333): the canonical 256-leaf tree ------------------
// Leaf l < 256 is the in-order sum of rows l, l + 256, l + 512, ...; then red[l] + red[l + 128],
// red[t] + red[t + 64] and the shuffle tree.  A row past the node's end adds +0.0, an identity on
// a sum that starts at +0.0.
__device__ __forceinline__ double wave_tree_sum(double x) {  // lane 0 holds the sum
#pragma unroll
  for (int k = 32; k >= 1; k >>= 1) x = x + __shfl_down(x, k, 64);
  return x;
}
// The tree above its leaves, by a workgroup whose lanes tid < 256 hold them in red[] (written
// before a barrier): valid in lane 0.  Every lane of the workgroup calls it (one barrier inside).
__device__ __forceinline__ double block_tree_sum(double *red, int tid) {
  if (tid < 128) red[tid] = red[tid] + red[tid + 128];
  __syncthreads();
  return tid < 64 ? wave_tree_sum(red[tid] + red[tid + 64]) : 0.0;
}
// The whole tree by ONE wave over kRows staged rows (t: the lane): lane t holds leaves t, t + 64,
// t + 128, t + 192 — the same additions in the same order.  Up to 4 LDS reads in flight
// (r < kRows: in bounds).  Valid in lane 0.
template <int kRows>
__device__ __forceinline__ double node_delta_tree64(const double *s_d, uint32_t t, uint32_t rows) {
  constexpr int kU = kRows / kTree, kB = kU < 4 ? kU : 4;
  double leaf[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    double sum = 0.0;
#pragma unroll
    for (int u0 = 0; u0 < kU; u0 += kB) {
      double v[kB];
#pragma unroll
      for (int u = 0; u < kB; ++u) v[u] = s_d[t + 64u * q + static_cast<uint32_t>(kTree) * (u0 + u)];
#pragma unroll
      for (int u = 0; u < kB; ++u) {
        const uint32_t r = t + 64u * q + static_cast<uint32_t>(kTree) * (u0 + u);
        sum = sum + (r < rows ? v[u] : 0.0);
      }
    }
    leaf[q] = sum;
  }
  return wave_tree_sum((leaf[0] + leaf[2]) + (leaf[1] + leaf[3]));
}

// ---- an aggregate's outputs ------------------------------------------------------------------------
// container.go:106-140 / vm.go:78-109 / pod.go:87-118 (a pod guards on Power, pod.go:96): the
// row's new totals E and powers P from its Δ and previous totals, stored at its slot.
template <int Z, bool NT>
__device__ __forceinline__ void aggregate_row(const DevState &st, const Attr<Z> &a, uint32_t role, uint32_t word,
                                              double delta, const uint64_t (&prev)[Z], uint32_t node,
                                              uint64_t (&E)[Z], double (&P)[Z]) {
  const double ratio =
      attribute_row<Z>(a, role == 3 ? a.live_pod : a.live, delta, (word & KACC_SLOT_NEW) != 0, prev, E, P);
  store_agg<Z, NT>(st, role, word & KACC_SLOT_MASK, E, P, ratio, node);
}
// The same with a pod's export (batch pod q); a pod whose slot is out of range (!ok) exports zeros.
template <int Z, bool NT>
__device__ __forceinline__ void aggregate_out(const kacc_interval &b, const DevState &st, const Attr<Z> &a,
                                              uint32_t role, uint32_t word, bool ok, double delta,
                                              const uint64_t (&prev)[Z], uint32_t node, uint32_t q) {
  if (!ok) {
    if (role == 3) export_pod_zero<Z>(b, q, st.err);
    return;
  }
  uint64_t E[Z];
  double P[Z];
  aggregate_row<Z, NT>(st, a, role, word, delta, prev, node, E, P);
  if (role == 3) export_pod<Z>(b, q, E, P, st.err);
}

}  // namespace kacc
