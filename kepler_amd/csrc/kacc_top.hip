// Top-K consumers of the RUNNING workloads, selected on the device.
//
// No reference counterpart: Kepler exports every running workload and leaves
// "which draw the most" to PromQL's topk; a fleet engine exports a selection.
// The rows are those of the caller's last interval batch (one workload kind);
// the value of a row is its slot's element of the table in `zone`: an energy
// word, a stored pod power, or the derived power ratio[slot] · ActivePower[node]
// under the guard of kacc_derive.hpp.  The rows' view, the order rule's key and the
// host's resolver are the shared row layer's (kacc_rows.hpp); the value path is this
// file's own: a segment knows its node, so the guard operands are loaded once per
// node into LDS and KACC_T_*_NODE is not gathered (the same bits for rows of the
// node's last processed interval: the validity rule of the derived tables).
//
// Order (the header's rule): descending key, equal keys in ascending batch row
// order.  The kernels sort ascending by (~key, row): three 32-bit compares, no
// 64-bit compare in the loop.
//
// One kernel, three uses:
//   per-node lists   one workgroup per node streams the node's rows
//   fleet stage 1    one workgroup per kGroup nodes -> a candidate list of <= k
//                    (~key, row, node) entries
//   fleet stage 2    one workgroup per `fan` candidate lists -> one list, repeated
//                    until at most `fan` are left; the last pass writes the outputs
// A workgroup keeps a 2048-entry LDS buffer: [0, kept) the best so far, sorted;
// new entries are appended behind them, and once `kept` == k only entries that
// beat the current k-th (the threshold) are appended at all.  When the buffer
// passes its trigger it is sorted (bitonic, over the next power of two >= its
// fill) and cut back to k.  The workgroup's sources (its nodes' rows, its lists'
// entries) are one index space walked in steps of what the buffer has room for.
// Nothing of a node lives in registers across that loop.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kacc_derive.hpp"
#include "kacc_internal.hpp"
#include "kacc_rows.hpp"

namespace kacc {
namespace top {

constexpr uint32_t kBuf = 2048;        // LDS buffer entries
constexpr uint32_t kMinTake = 256;     // room left in the buffer when it is sorted again
constexpr uint32_t kGroup = 8;        // nodes per workgroup in fleet stage 1
constexpr uint32_t kMinFan = 8;        // candidate lists per workgroup in stage 2, at least
constexpr uint32_t kErrTop = 1u << 9;  // a slot past the capacity or a row range outside the batch
constexpr uint32_t kNone = 0xffffffffu;

using rows::kDerived, rows::kEnergy, rows::kStored, rows::power_key;  // where entries come from: a table,
constexpr int kCand = 3;                                               // or candidate lists
enum Out { kNodes = 0, kList = 1, kFleet = 2 };                   // where the kept entries go
// Threads per workgroup.  A node's selection is one dependent chain (loads, sort, loads), so the
// per-node lists pay in workgroups per CU: six of 256 threads (their LDS) against four of 512.
// The fleet's workgroups stream many rows each and sort full buffers: 512.
constexpr int threads_of(int out) { return out == kNodes ? 256 : 512; }

struct Cand {  // candidate lists: list l holds count[l] <= k entries at [l * k, ...)
  uint2 *ikey;  // ~key: .y high word, .x low word
  uint32_t *row;
  uint32_t *node;
  uint32_t *count;
};

struct Args {
  rows::View v;  // the rows (no node mask, no flag words: the guard operands go through LDS)
  // the table
  const uint64_t *words;  // energy / stored power words of `zone`: words[slot * v.tab_stride]
  uint32_t mode;          // Src of the table (the value of an emitted entry)
  uint32_t zone;
  // selection
  uint32_t k;
  uint32_t group;    // sources (nodes or lists) per workgroup
  uint32_t n_lists;  // kCand: lists in `in`
  Cand in, out;
  uint32_t *out_count, *out_row, *out_slot, *out_node;
  uint64_t *out_value;
  uint32_t *err;
};

struct NodeGuard {  // the node's operands of the guard (process.go:124), loaded once per node
  double aP;
  bool live;
};
__device__ __forceinline__ NodeGuard node_guard(const ProcDerive &d, uint32_t n, uint32_t zone) {
  const uint64_t i = static_cast<uint64_t>(n) * d.zones + zone;
  NodeGuard g;
  g.aP = d.active_power[i];
  g.live = !(d.active_energy[i] == 0 || !(d.cpu_delta[n] != 0) || !(g.aP != 0));
  return g;
}

// The table's own value of slot s (bits of the f64 for a power table).
template <int kSrc>
__device__ __forceinline__ uint64_t slot_value(const Args &a, uint64_t s, const NodeGuard &g) {
  if constexpr (kSrc == kDerived) {
    return static_cast<uint64_t>(__double_as_longlong(g.live ? a.v.pd.ratio[s] * g.aP : 0.0));
  } else {
    return a.words[s * a.v.tab_stride];
  }
}

// (hi, lo, row) ascending: true when a sorts after b
__device__ __forceinline__ bool after(uint2 ak, uint32_t ar, uint2 bk, uint32_t br) {
  return ak.y != bk.y ? ak.y > bk.y : (ak.x != bk.x ? ak.x > bk.x : ar > br);
}

template <int kSrc, int kOut>
__global__ __launch_bounds__(threads_of(kOut)) void select_kernel(const Args a) {
  constexpr uint32_t kThreads = threads_of(kOut), kPer = kBuf / kThreads;  // kPer: entries a thread loads per step
  constexpr bool kCarry = kOut != kNodes;  // entries carry their node
  __shared__ uint2 s_key[kBuf];
  __shared__ uint32_t s_row[kBuf];
  __shared__ uint32_t s_node[kCarry ? kBuf : 1];
  __shared__ uint32_t s_fill;
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t k = a.k;
  // without a threshold yet the first sort comes early for a small k: what passes
  // the threshold afterwards is a small share of the rows
  uint32_t first_trigger = 256;
  while (first_trigger < 4 * k && first_trigger < kBuf) first_trigger <<= 1;

  uint32_t fill = 0, kept = 0;  // buffer entries, sorted prefix (both workgroup-uniform)
  bool have_thr = false;
  uint2 thr_key = make_uint2(kNone, kNone);
  uint32_t thr_row = kNone;
  if (tid == 0) s_fill = 0;
  __syncthreads();

  auto sort_and_cut = [&]() {  // [0, fill) sorted, cut to k; sets the threshold
    uint32_t P = 64;
    while (P < fill) P <<= 1;
    for (uint32_t i = fill + tid; i < P; i += kThreads) {
      s_key[i] = make_uint2(kNone, kNone);
      s_row[i] = kNone;
    }
    __syncthreads();
    for (uint32_t sz = 2; sz <= P; sz <<= 1) {
      for (uint32_t st = sz >> 1; st > 0; st >>= 1) {
        for (uint32_t t = tid; t < (P >> 1); t += kThreads) {
          const uint32_t i = 2 * t - (t & (st - 1)), j = i + st;
          const uint2 ki = s_key[i], kj = s_key[j];
          const uint32_t ri = s_row[i], rj = s_row[j];
          const bool up = (i & sz) == 0;
          if (after(ki, ri, kj, rj) == up) {
            s_key[i] = kj;
            s_key[j] = ki;
            s_row[i] = rj;
            s_row[j] = ri;
            if constexpr (kCarry) {
              const uint32_t ni = s_node[i];
              s_node[i] = s_node[j];
              s_node[j] = ni;
            }
          }
        }
        // a step of stride <= 64 pairs elements inside one 128-entry block, and a wave owns
        // the same blocks in every step: only a step of a longer stride, or the step before
        // one, needs the workgroup's barrier
        const uint32_t next = st > 1 ? (st >> 1) : (sz < P ? sz : kBuf);
        if (st > 64 || next > 64) {
          __syncthreads();
        } else {
          rows::wave_lds_fence();
        }
      }
    }
    fill = kept = min(fill, k);
    if (kept == k) {
      have_thr = true;
      thr_key = s_key[k - 1];
      thr_row = s_row[k - 1];  // appends land at [k, ...): it stays put
    }
    if (tid == 0) s_fill = fill;
    __syncthreads();
  };

  // append the entries that beat the threshold (any order: the sort is a total order)
  auto append = [&](bool ok, uint2 key, uint32_t row, uint32_t node) {
    const bool pass = ok && after(thr_key, thr_row, key, row);
    const uint64_t m = __ballot(pass);
    if (m == 0) return;
    uint32_t base = 0;
    if (lane == static_cast<uint32_t>(__ffsll(static_cast<long long>(m)) - 1))
      base = atomicAdd(&s_fill, static_cast<uint32_t>(__popcll(m)));
    base = __shfl(base, __ffsll(static_cast<long long>(m)) - 1, 64);
    if (pass) {
      const uint32_t p = base + static_cast<uint32_t>(__popcll(m & ((1ull << lane) - 1ull)));
      s_key[p] = key;
      s_row[p] = row;
      if constexpr (kCarry) s_node[p] = node;
    }
  };

  // ---- the workgroup's sources as ONE index space ---------------------------------------
  // nodes: index f is row s_r0[n] + (f - s_pre[n]) of the group's node n, the listed nodes'
  // rows back to back (a read-error node and a row range outside the batch count no rows);
  // candidate lists: f = list * k + j, entries past the list's count skipped.  A step takes
  // what the buffer has room for, whichever nodes or lists it spans: no per-source latency.
  __shared__ uint32_t s_pre[kGroup + 1], s_r0[kGroup];
  __shared__ double s_aP[kGroup];
  __shared__ uint32_t s_live[kGroup];
  const uint32_t n_src = kSrc == kCand ? a.n_lists : a.v.n_nodes;
  const uint32_t src0 = static_cast<uint32_t>(min(static_cast<uint64_t>(blockIdx.x) * a.group, static_cast<uint64_t>(n_src)));
  const uint32_t ng = min(a.group, n_src - src0);
  uint32_t total;
  if constexpr (kSrc == kCand) {
    total = ng * k;  // <= fan * k
  } else {
    if (tid < ng) {  // ng <= kGroup; every load issued before the first use: one round trip
      const uint32_t n = src0 + tid;
      const uint32_t r0 = a.v.row_off[n], r1 = a.v.row_off[n + 1];
      const uint32_t status = a.v.node_status ? a.v.node_status[n] : 0u;
      NodeGuard g{0.0, false};
      if constexpr (kSrc == kDerived) g = node_guard(a.v.pd, n, a.zone);
      uint32_t cnt = 0;
      if (r0 > r1 || r1 > a.v.n_rows)
        atomicOr(a.err, kErrTop);  // left out
      else if (!(status & KACC_NODE_READ_ERROR))
        cnt = r1 - r0;
      s_r0[tid] = r0;
      s_pre[tid + 1] = cnt;
      s_aP[tid] = g.aP;
      s_live[tid] = g.live;
    }
    __syncthreads();
    if (tid == 0) {
      uint32_t run = 0;
      s_pre[0] = 0;
      for (uint32_t n = 0; n < ng; ++n) {
        uint32_t cnt = s_pre[n + 1];
        if (cnt > kNone - run) {  // overlapping ranges of a bad batch: left out
          atomicOr(a.err, kErrTop);
          cnt = 0;
        }
        run += cnt;
        s_pre[n + 1] = run;
      }
    }
    __syncthreads();
    total = s_pre[ng];
  }
  uint32_t pos = 0;
  while (pos < total) {
    const uint32_t limit = have_thr ? kBuf : first_trigger;
    const uint32_t take = min(limit - fill, total - pos);  // fill < limit here
    // take <= kBuf = kPer * kThreads.  No load sits behind a branch: an index past the step
    // is clamped to the step's last one and a bad slot to slot 0, so a thread's kPer loads
    // of one kind are in flight together (two round trips per step, not two per entry).
    bool ok[kPer];
    uint2 key[kPer];
    uint32_t row[kPer], node[kPer];
    const uint32_t last = pos + take - 1;
    if constexpr (kSrc == kCand) {
      uint32_t j[kPer], cnt[kPer];
      uint64_t e[kPer];
#pragma unroll
      for (uint32_t u = 0; u < kPer; ++u) {
        const uint32_t i = u * kThreads + tid, f = min(pos + i, last);
        const uint32_t l = f / k;
        j[u] = f - l * k;
        ok[u] = i < take;
        e[u] = static_cast<uint64_t>(src0 + l) * k;
        cnt[u] = a.in.count[src0 + l];
      }
#pragma unroll
      for (uint32_t u = 0; u < kPer; ++u) {
        ok[u] = ok[u] && j[u] < min(cnt[u], k);
        e[u] += ok[u] ? j[u] : 0u;  // a list's first entry is always allocated
        key[u] = a.in.ikey[e[u]];
        row[u] = a.in.row[e[u]];
        node[u] = a.in.node[e[u]];
      }
    } else {
      uint32_t w[kPer], ln[kPer];
#pragma unroll
      for (uint32_t u = 0; u < kPer; ++u) {
        const uint32_t i = u * kThreads + tid, f = min(pos + i, last);
        uint32_t n = 0;
        for (uint32_t s = 1; s < ng; ++s) n += f >= s_pre[s];
        ok[u] = i < take;
        ln[u] = n;
        row[u] = s_r0[n] + (f - s_pre[n]);
        node[u] = src0 + n;
        w[u] = a.v.slot[row[u]];
      }
      uint64_t v[kPer];
      bool bad = false;
#pragma unroll
      for (uint32_t u = 0; u < kPer; ++u) {
        const uint64_t sl = w[u] & KACC_SLOT_MASK;
        const bool in = sl < a.v.cap;
        bad = bad || (ok[u] && !in);  // left out
        ok[u] = ok[u] && in;
        v[u] = 0;
        if (a.v.cap != 0) {  // uniform
          if constexpr (kSrc == kDerived)
            v[u] = static_cast<uint64_t>(__double_as_longlong(a.v.pd.ratio[in ? sl : 0]));
          else
            v[u] = a.words[(in ? sl : 0) * a.v.tab_stride];
        }
      }
      if (bad) atomicOr(a.err, kErrTop);
#pragma unroll
      for (uint32_t u = 0; u < kPer; ++u) {
        if constexpr (kSrc == kDerived) {
          const double p = s_live[ln[u]] ? __longlong_as_double(static_cast<long long>(v[u])) * s_aP[ln[u]] : 0.0;
          v[u] = static_cast<uint64_t>(__double_as_longlong(p));
        }
        const uint64_t ik = ~(kSrc == kEnergy ? v[u] : power_key(v[u]));
        key[u] = make_uint2(static_cast<uint32_t>(ik), static_cast<uint32_t>(ik >> 32));
      }
    }
#pragma unroll
    for (uint32_t u = 0; u < kPer; ++u)
      if (u * kThreads < take) append(ok[u], key[u], row[u], node[u]);  // workgroup-uniform
    pos += take;
    __syncthreads();
    fill = s_fill;
    __syncthreads();  // everyone has read it before the next appends move it
    // with a threshold: sort when fewer than kMinTake entries of room are left (a sort costs
    // ten load steps: few sorts of a full buffer, steps of at least kMinTake entries)
    const uint32_t trigger = have_thr ? kBuf - kMinTake : first_trigger;
    if (fill >= trigger) sort_and_cut();
  }
  if (fill > kept) sort_and_cut();
  const uint32_t count = min(fill, k);

  // ---- the kept entries leave --------------------------------------------------------
  if constexpr (kOut == kList) {
    const uint64_t o = static_cast<uint64_t>(blockIdx.x) * k;
    if (tid == 0) a.out.count[blockIdx.x] = count;
    for (uint32_t j = tid; j < count; j += kThreads) {
      a.out.ikey[o + j] = s_key[j];
      a.out.row[o + j] = s_row[j];
      a.out.node[o + j] = s_node[j];
    }
  } else {
    const uint64_t o = static_cast<uint64_t>(blockIdx.x) * k;  // kFleet: one workgroup
    if (tid == 0) a.out_count[blockIdx.x] = count;
    for (uint32_t j = tid; j < k; j += kThreads) {
      uint32_t row = kNone, sl = kNone, node = kNone;
      uint64_t v = 0;
      if (j < count) {
        row = s_row[j];
        node = kOut == kFleet ? s_node[j] : blockIdx.x;
        sl = a.v.slot[row] & KACC_SLOT_MASK;  // < cap: checked when the row entered
        if (a.mode == kDerived)
          v = slot_value<kDerived>(a, sl, node_guard(a.v.pd, node, a.zone));
        else
          v = a.words[static_cast<uint64_t>(sl) * a.v.tab_stride];
      }
      a.out_row[o + j] = row;
      if (a.out_slot) a.out_slot[o + j] = sl;
      if (kOut == kFleet && a.out_node) a.out_node[o + j] = node;
      if (a.out_value) a.out_value[o + j] = v;
    }
  }
}

}  // namespace top
}  // namespace kacc

namespace {

using kacc::top::Args;

int fill_args(kacc_ctx *ctx, const char *fn, kacc_table t, uint32_t zone, uint32_t k, const kacc_top_rows *rows,
              const void *out_count, const void *out_row, Args *a) {
  kacc::rows::Table tab;
  *a = Args{};
  int rc = kacc::rows::resolve_table(ctx, fn, t, zone, &tab);
  if (rc != KACC_OK) return rc;
  if (k < 1 || k > KACC_TOP_MAX) return kacc_fail(ctx, KACC_EINVAL, "%s: k = %u outside 1 .. %u", fn, k, KACC_TOP_MAX);
  if (!rows || !out_count || !out_row) return kacc_fail(ctx, KACC_EINVAL, "%s: NULL argument", fn);
  if ((rc = kacc::rows::resolve(ctx, fn, tab.kind, rows, nullptr, &a->v)) != KACC_OK) return rc;
  a->mode = tab.src;
  a->words = tab.words;
  a->zone = zone;
  a->k = k;
  a->err = ctx->d_err;
  return KACC_OK;
}

template <int kOut>
void launch_rows(const Args &a, uint32_t grid, hipStream_t st) {
  using namespace kacc::top;
  kacc::rows::dispatch_src(a.mode, [&](auto s) {
    KACC_LAUNCH((select_kernel<s(), kOut>), dim3(grid), dim3(threads_of(kOut)), 0, st, a);
  });
}

}  // namespace

extern "C" {

int kacc_top_nodes(kacc_ctx *ctx, kacc_table t, uint32_t zone, uint32_t k, const kacc_top_rows *rows,
                   uint32_t *out_count, uint32_t *out_row, uint32_t *out_slot, uint64_t *out_value, void *stream) {
  if (!ctx) return KACC_EINVAL;
  Args a;
  kacc::rows::Call call(ctx, "kacc_top_nodes");
  int rc = fill_args(ctx, call.fn, t, zone, k, rows, out_count, out_row, &a);
  if (rc != KACC_OK) return rc;
  if (a.v.n_nodes == 0) return KACC_OK;
  if (a.v.n_nodes > 0x7fffffffu) return kacc_fail(ctx, KACC_EINVAL, "kacc_top_nodes: too many nodes for one launch");
  if ((rc = call.open(stream)) != KACC_OK) return rc;
  a.group = 1;
  a.out_count = out_count;
  a.out_row = out_row;
  a.out_slot = out_slot;
  a.out_value = out_value;
  launch_rows<kacc::top::kNodes>(a, a.v.n_nodes, call.st);
  KACC_HIP(ctx, hipGetLastError());
  return KACC_OK;
}

int kacc_top_fleet(kacc_ctx *ctx, kacc_table t, uint32_t zone, uint32_t k, const kacc_top_rows *rows,
                   uint32_t *out_count, uint32_t *out_row, uint32_t *out_slot, uint32_t *out_node,
                   uint64_t *out_value, void *stream) {
  using namespace kacc::top;
  if (!ctx) return KACC_EINVAL;
  Args a;
  kacc::rows::Call call(ctx, "kacc_top_fleet");
  int rc = fill_args(ctx, call.fn, t, zone, k, rows, out_count, out_row, &a);
  if (rc != KACC_OK || (rc = call.open(stream)) != KACC_OK) return rc;
  hipStream_t st = call.st;
  // stage 1 leaves L1 lists in A; the passes of stage 2 alternate between B and A
  const uint32_t fan = std::max(kMinFan, (2 * kBuf + k - 1) / k);  // >= 4096 candidates per workgroup
  const uint64_t L1 = (static_cast<uint64_t>(a.v.n_nodes) + kGroup - 1) / kGroup;
  const uint64_t L2 = (L1 + fan - 1) / fan;
  const uint64_t ents = (L1 + L2) * k, lists = L1 + L2;
  Cand A;  // both stages' lists: B's follow A's in every array
  kacc::plan::Layout tmp;
  tmp.add(&A.ikey, ents);
  for (uint32_t **p : {&A.row, &A.node}) tmp.add(p, ents);
  tmp.add(&A.count, lists);
  if ((rc = call.alloc(tmp, 16)) != KACC_OK) return rc;
  const Cand B{A.ikey + L1 * k, A.row + L1 * k, A.node + L1 * k, A.count + L1};
  if (L1) {
    a.group = kGroup;
    a.out = A;
    launch_rows<kList>(a, static_cast<uint32_t>(L1), st);
  }
  uint64_t L = L1;
  Cand in = A, out = B;
  while (L > fan) {
    const uint64_t Ln = (L + fan - 1) / fan;
    a.group = fan;
    a.n_lists = static_cast<uint32_t>(L);
    a.in = in;
    a.out = out;
    KACC_LAUNCH((select_kernel<kCand, kList>), dim3(static_cast<uint32_t>(Ln)), dim3(threads_of(kList)), 0, st, a);
    std::swap(in, out);
    L = Ln;
  }
  a.group = fan;
  a.n_lists = static_cast<uint32_t>(L);
  a.in = in;
  a.out_count = out_count;
  a.out_row = out_row;
  a.out_slot = out_slot;
  a.out_node = out_node;
  a.out_value = out_value;
  KACC_LAUNCH((select_kernel<kCand, kFleet>), dim3(1), dim3(threads_of(kFleet)), 0, st, a);
  KACC_HIP(ctx, hipGetLastError());
  return KACC_OK;
}

}  // extern "C"
