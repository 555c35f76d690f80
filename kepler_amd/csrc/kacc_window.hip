// Energy over a caller-defined window, summed by group, on the device.
//
// No reference call is replaced: Kepler exports joule counters and leaves
// `sum by (label)(increase(kepler_*_joules_total[w]))` to PromQL; it exports its terminated
// workloads so that their last joules reach that query (terminated_resource_tracker.go,
// process.go:87-99).  A window keeps, per slot of one workload kind, the slot's EnergyTotal at
// the window's start (`base`) and the group of the slot's workload (`slot_group`), and per group
// what the workloads that terminated inside the window used in it (`retired`, `retired_count`).
// Every result is an integer sum mod 2^64: the same bytes for any tiling, row order, shard split
// or number of GPUs.
//
// The rows, their nodes' flag words and the tile prelude are the shared row layer's
// (kacc_rows.hpp); this file adds the window's state on top.
//
//   retire     (step, phase a) a wave per node of the join's terminated segments, 64 slots a
//              round: a lane takes its slot's group with an exchange (a slot retires once), loads
//              the slot's two records and adds E - base into its group's words.  Atomics on ONE
//              word serialise at the memory side (about 10 ns each), so the words are the
//              workgroup's LDS bins while G (1 + Z) of them fit - 128 persistent 1,024-thread
//              workgroups, flushed with one atomic per non-zero word - and beyond that the
//              window's own, where the lanes of a group that fills much of a wave add up in
//              the wave first (ballot, then a masked wave sum)
//   adopt      (step, phase b) one workgroup per tile of batch rows (the shared prelude): the
//              4-byte slot words are streamed; a listed NEW row (every listed row under
//              KACC_WINDOW_ASSIGN_ALL) stores its id, a NEW row zeroes its base
//   mark       base = E for every slot (a copy; a gather out of the pods' 2Z-word records)
//   node_prep  the shared layer's: one flag word per node
//   read       persistent workgroups over tiles of batch rows: every row's slot word, its
//              slot's id and its two Z-word records are loaded (clamped, none behind a
//              data-dependent branch), E - base goes to out_row and, for a row with a group,
//              into the group's bins: in LDS (replicated per lane subset while they fit the
//              small size, else one copy) and flushed with one atomic per workgroup and
//              word, or - more groups than LDS holds - with u64 atomics straight into the
//              accumulator
//   finish     one thread per accumulator word: the outputs
// Every index is clamped (the shared layer's rules; terminated slots and counts here), so no
// input faults.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kacc_internal.hpp"
#include "kacc_rows.hpp"

namespace kacc {
namespace win {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kAdoptPer = 8;                       // adopt: rows per lane and tile
constexpr uint32_t kAdoptTile = kThreads * kAdoptPer;
constexpr uint32_t kReadPer = 4;                        // read: rows per lane and tile, their records in flight together
constexpr uint32_t kReadTile = kThreads * kReadPer;
constexpr uint32_t kSmallWords = 4096;                  // u64 of LDS bins: 32 KiB, three workgroups per CU
constexpr uint32_t kBigWords = 9984;                    // 78 KiB, two workgroups per CU: 1,996 groups at Z = 4
static_assert(kSmallWords == plan::kWindowLds.small_words && kBigWords == plan::kWindowLds.big_words,
              "the host plans the read with the kernels' LDS sizes");
constexpr uint32_t kRetireThreads = 1024;               // retire: 16 waves, each takes a node at a time
constexpr uint32_t kRetireWaves = kRetireThreads / 64;
constexpr uint32_t kRetireGrid = 128;                   // retire: persistent workgroups while the bins are in LDS
constexpr uint32_t kWaveSum = 8;                        // retire: lanes of one group at or past this add up in the wave
constexpr uint32_t kMergeRounds = 4;                    // retire: groups tried for that per 64 slots (the digit merges' four)
constexpr uint32_t kErrGroup = 1u << 13;                // "group sums": a slot, an id, a count or a row range past its range
using rows::kCus, rows::lds_add;
using u64x2 = __attribute__((ext_vector_type(2))) unsigned long long;

struct State {  // a window's arrays and the records of its kind
  uint64_t *base;           // [cap * Z]
  uint32_t *slot_group;     // [cap]
  uint64_t *retired;        // [G * Z]
  uint32_t *retired_count;  // [G]
  const uint64_t *tab_e;    // the kind's energy table
  uint32_t tab_stride;      // Z, or 2Z for the pod records
  uint32_t Z, n_groups;
  uint64_t cap;
  uint32_t *err;
};

__device__ __forceinline__ void global_add(uint64_t *p, uint64_t v) {
  atomicAdd(reinterpret_cast<unsigned long long *>(p), static_cast<unsigned long long>(v));
}

// The sum of v over all 64 lanes, in every lane: every lane of the wave must be active (the
// callers' loops are wave-uniform); a lane outside the caller's set passes 0.
__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
  for (uint32_t off = 32; off > 0; off >>= 1) v += __shfl_xor(static_cast<unsigned long long>(v), off, 64);
  return v;
}

// ---- step (a): retire -----------------------------------------------------------------------

struct RetireArgs {
  State w;
  uint32_t n_nodes;
  const uint32_t *slot_off, *term_slot, *term_count;
  uint32_t merge_rounds;  // the global variant's wave merges per 64 slots: kMergeRounds (a knob: 0 .. 64)
};

// kLds: the groups' words - [G] counts, [G * Z] sums - fit kBigWords of LDS: a few persistent
// workgroups, every wave takes nodes in turn and adds into the workgroup's bins, flushed with one
// atomic per non-zero word.  Else one node per wave and the atomics go straight to the window.
template <bool kLds>
__global__ __launch_bounds__(kRetireThreads) void retire_kernel(const RetireArgs a) {
  __shared__ uint64_t s_bin[kLds ? kBigWords : 1u];
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
  const uint32_t Z = a.w.Z, G = a.w.n_groups;
  if constexpr (kLds) {
    for (uint32_t i = threadIdx.x; i < G * (1u + Z); i += kRetireThreads) s_bin[i] = 0;  // <= kBigWords (host)
    __syncthreads();
  }
  bool bad = false;
  for (uint32_t n = blockIdx.x * kRetireWaves + wv; n < a.n_nodes; n += gridDim.x * kRetireWaves) {  // wave-uniform
    const uint32_t b0 = a.slot_off[n], seg = a.slot_off[n + 1] - b0;
    uint32_t c = a.term_count[n];
    if (c > seg) {  // wave-uniform: a count past the segment leaves the node's list out
      bad = true;
      c = 0;
    }
    for (uint32_t c0 = 0; c0 < c; c0 += 64) {  // wave-uniform
      const bool in = c0 + lane < c;
      const uint32_t s = a.term_slot[b0 + min(c0 + lane, c - 1u)];
      const bool valid = in && s < a.w.cap;
      bad = bad || (in && !valid);
      const uint32_t sl = valid ? s : 0u;
      // the slot's two records at the clamped slot, every word in flight beside the exchange: no
      // load sits behind the validity test
      const uint64_t *se = a.w.tab_e + static_cast<uint64_t>(sl) * a.w.tab_stride;
      const uint64_t *sb = a.w.base + static_cast<uint64_t>(sl) * Z;
      uint64_t d[KACC_MAX_ZONES];
#pragma unroll
      for (uint32_t z = 0; z < KACC_MAX_ZONES; ++z) d[z] = (z < Z && a.w.cap != 0) ? se[z] - sb[z] : 0ull;  // uniform
      // the slot leaves the window: whoever takes its id retires it, once
      const uint32_t g = valid ? atomicExch(&a.w.slot_group[sl], KACC_GROUP_NONE) : KACC_GROUP_NONE;
      bool live = g < G;
      if constexpr (kLds) {
        if (live) {
          lds_add(&s_bin[g], 1ull);
#pragma unroll
          for (uint32_t z = 0; z < KACC_MAX_ZONES; ++z)
            if (z < Z && d[z]) lds_add(&s_bin[G + g * Z + z], d[z]);
        }
      } else {
        // a few rounds, each for the group of the first lane not yet tried: a group with many
        // lanes in the wave adds up in the wave and sends one atomic per word
        bool cand = live;
        for (uint32_t round = 0; round < a.merge_rounds; ++round) {  // uniform
          const uint64_t todo = __ballot(cand);
          if (todo == 0) break;  // wave-uniform
          const uint32_t lead = static_cast<uint32_t>(__builtin_ctzll(todo));
          const uint32_t g0 = __shfl(g, lead, 64);
          const bool mine = cand && g == g0;
          const uint32_t cnt = static_cast<uint32_t>(__popcll(__ballot(mine)));
          cand = cand && !mine;
          if (cnt < kWaveSum) continue;  // wave-uniform: its lanes stay live and send their own below
#pragma unroll
          for (uint32_t z = 0; z < KACC_MAX_ZONES; ++z) {
            if (z >= Z) break;  // uniform
            const uint64_t sum = wave_sum(mine ? d[z] : 0ull);
            if (lane == lead && sum) global_add(&a.w.retired[static_cast<uint64_t>(g0) * Z + z], sum);
          }
          if (lane == lead) atomicAdd(&a.w.retired_count[g0], cnt);
          live = live && !mine;
        }
        if (live) {  // the rest, each lane its own: no-return atomics, all in flight together
#pragma unroll
          for (uint32_t z = 0; z < KACC_MAX_ZONES; ++z)
            if (z < Z && d[z]) global_add(&a.w.retired[static_cast<uint64_t>(g) * Z + z], d[z]);
          atomicAdd(&a.w.retired_count[g], 1u);
        }
      }
    }
  }
  if (__ballot(bad) != 0 && lane == 0) atomicOr(a.w.err, kErrGroup);  // one lane of the wave
  if constexpr (kLds) {
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < G * (1u + Z); i += kRetireThreads) {
      const uint64_t v = s_bin[i];
      if (v == 0) continue;
      if (i < G)
        atomicAdd(&a.w.retired_count[i], static_cast<uint32_t>(v));
      else
        global_add(&a.w.retired[i - G], v);
    }
  }
}

// ---- step (b): adopt ------------------------------------------------------------------------

struct AdoptArgs {
  State w;
  rows::View v;
  const uint32_t *group;  // [n_rows] or NULL: group 0
  uint32_t assign_all;
};

__global__ __launch_bounds__(kThreads) void adopt_kernel(const AdoptArgs a) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t Z = a.w.Z;
  rows::Located<kAdoptPer> t;
  rows::locate<kAdoptPer>(a.v, nullptr, blockIdx.x, kAdoptTile, lane, wave, t);
#pragma unroll
  for (uint32_t u = 0; u < kAdoptPer; ++u) rows::check_row(a.v, 1u, t, u);
  bool bad = t.bad;
  bool fresh[kAdoptPer], act[kAdoptPer];
  uint32_t g[kAdoptPer];
#pragma unroll
  for (uint32_t u = 0; u < kAdoptPer; ++u) {
    fresh[u] = t.ok[u] && (t.w[u] & KACC_SLOT_NEW);
    act[u] = fresh[u] || (t.ok[u] && a.assign_all);
    g[u] = 0u;
  }
  if (a.group) {  // uniform; a row that stores no id reads the batch's row 0: no load behind a branch
#pragma unroll
    for (uint32_t u = 0; u < kAdoptPer; ++u) g[u] = a.group[act[u] ? t.r[u] : 0u];
  }
#pragma unroll
  for (uint32_t u = 0; u < kAdoptPer; ++u) {
    bool bad_id;
    const bool gin = rows::group_ok(g[u], a.w.n_groups, bad_id);
    bad = bad || (act[u] && bad_id);
    if (act[u]) a.w.slot_group[t.sl[u]] = gin ? g[u] : KACC_GROUP_NONE;
    if (fresh[u]) {
      uint64_t *sb = a.w.base + static_cast<uint64_t>(t.sl[u]) * Z;
      for (uint32_t z = 0; z < Z; ++z) sb[z] = 0;
    }
  }
  if (bad) atomicOr(a.w.err, kErrGroup);
}

// ---- mark -----------------------------------------------------------------------------------

// base[s * Z + z] = E[s * stride + z].  kVec: stride == Z and Z even, 16 bytes per thread and step.
template <bool kVec>
__global__ __launch_bounds__(kThreads) void mark_kernel(const State w, uint64_t n) {
  const uint64_t step = static_cast<uint64_t>(gridDim.x) * kThreads;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; i < n; i += step) {
    if constexpr (kVec) {
      reinterpret_cast<u64x2 *>(w.base)[i] = reinterpret_cast<const u64x2 *>(w.tab_e)[i];
    } else {
      const uint64_t s = i / w.Z, z = i - s * w.Z;
      w.base[i] = w.tab_e[s * w.tab_stride + z];
    }
  }
}

// ---- read -----------------------------------------------------------------------------------

struct ReadArgs {
  State w;
  rows::View v;
  uint32_t tiles, splits;
  uint32_t copies, copy_stride;  // LDS bins: 2^k copies, copy_stride u64 apart
  uint64_t *acc;                 // [G] count, [G * Z] running
  uint32_t *out_count, *out_retired_count;
  uint64_t *out_running, *out_retired, *out_total, *out_row;
};

// kZ: the zone count when it is 4 (16-byte loads and stores), else 0: any Z, word by word.
// kLds: the LDS words of the bins; 0: the accumulator itself, with global atomics.
template <uint32_t kZ, uint32_t kLds>
__global__ __launch_bounds__(kThreads, kLds == kBigWords ? 2 : 3) void read_kernel(const ReadArgs a) {
  __shared__ uint64_t s_bin[kLds ? kLds : 1u];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t Z = kZ ? kZ : a.w.Z, G = a.w.n_groups;
  uint32_t b_off = 0;
  if constexpr (kLds != 0) {
    for (uint32_t i = tid; i < a.copies * a.copy_stride; i += kThreads) s_bin[i] = 0;  // <= kLds (host)
    __syncthreads();
    b_off = (lane & (a.copies - 1u)) * a.copy_stride;
  }
  auto add = [&](uint32_t i, uint64_t v) {  // word i of the bins: [G] counts, [G * Z] sums
    if constexpr (kLds != 0)
      lds_add(&s_bin[b_off + i], v);
    else
      global_add(&a.acc[i], v);
  };
  bool bad = false;
  for (uint32_t tile = blockIdx.x; tile < a.tiles; tile += a.splits) {  // workgroup-uniform
    rows::Located<kReadPer> t;
    rows::locate<kReadPer>(a.v, nullptr, tile, kReadTile, lane, wave, t);
#pragma unroll
    for (uint32_t u = 0; u < kReadPer; ++u) rows::check_row(a.v, 1u, t, u);
    bad = bad || t.bad;
    uint32_t g[kReadPer];
    if constexpr (kZ == 4) {
      u64x2 e[kReadPer][2], b[kReadPer][2];
#pragma unroll
      for (uint32_t u = 0; u < kReadPer; ++u) {  // every row's records, clamped: all in flight together
        e[u][0] = e[u][1] = b[u][0] = b[u][1] = u64x2{0ull, 0ull};
        g[u] = KACC_GROUP_NONE;
        if (a.w.cap != 0) {  // uniform
          const u64x2 *se = reinterpret_cast<const u64x2 *>(a.w.tab_e + static_cast<uint64_t>(t.sl[u]) * a.w.tab_stride);
          const u64x2 *sb = reinterpret_cast<const u64x2 *>(a.w.base + static_cast<uint64_t>(t.sl[u]) * 4u);
          g[u] = a.w.slot_group[t.sl[u]];
          e[u][0] = se[0];
          e[u][1] = se[1];
          b[u][0] = sb[0];
          b[u][1] = sb[1];
        }
      }
#pragma unroll
      for (uint32_t u = 0; u < kReadPer; ++u) {
        const u64x2 zero{0ull, 0ull};
        const u64x2 d0 = t.ok[u] ? e[u][0] - b[u][0] : zero, d1 = t.ok[u] ? e[u][1] - b[u][1] : zero;
        if (a.out_row && t.in_batch[u]) {  // out_row: uniform
          u64x2 *dst = reinterpret_cast<u64x2 *>(a.out_row + static_cast<uint64_t>(t.r[u]) * 4u);
          dst[0] = d0;
          dst[1] = d1;
        }
        if (t.ok[u] && g[u] < G) {
          add(g[u], 1ull);
          add(G + g[u] * 4u + 0u, d0.x);
          add(G + g[u] * 4u + 1u, d0.y);
          add(G + g[u] * 4u + 2u, d1.x);
          add(G + g[u] * 4u + 3u, d1.y);
        }
      }
    } else {
#pragma unroll
      for (uint32_t u = 0; u < kReadPer; ++u) g[u] = a.w.cap != 0 ? a.w.slot_group[t.sl[u]] : KACC_GROUP_NONE;
#pragma unroll
      for (uint32_t u = 0; u < kReadPer; ++u) {
        const uint64_t *se = a.w.tab_e + static_cast<uint64_t>(t.sl[u]) * a.w.tab_stride;
        const uint64_t *sb = a.w.base + static_cast<uint64_t>(t.sl[u]) * Z;
        const bool grouped = t.ok[u] && g[u] < G;
        for (uint32_t z = 0; z < Z; ++z) {
          const uint64_t d = (a.w.cap != 0 && t.ok[u]) ? se[z] - sb[z] : 0ull;  // cap: uniform; ok: a select
          if (a.out_row && t.in_batch[u]) a.out_row[static_cast<uint64_t>(t.r[u]) * Z + z] = d;
          if (grouped) add(G + g[u] * Z + z, d);
        }
        if (grouped) add(g[u], 1ull);
      }
    }
  }
  if (bad) atomicOr(a.w.err, kErrGroup);
  if constexpr (kLds != 0) {
    __syncthreads();
    // the flush: word i of the bins (the copies summed) into the accumulator, consecutive lanes
    // on consecutive words
    for (uint32_t i = tid; i < G * (1u + Z); i += kThreads) {
      uint64_t v = 0;
      for (uint32_t c = 0; c < a.copies; ++c) v += s_bin[c * a.copy_stride + i];
      if (v) global_add(&a.acc[i], v);
    }
  }
}

// Every non-NULL output of every group: the running part out of the accumulator, the retired
// part out of the window.
__global__ __launch_bounds__(kThreads) void finish_kernel(const ReadArgs a) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
  const uint64_t G = a.w.n_groups, GZ = G * a.w.Z;
  if (i < G) {
    if (a.out_count) a.out_count[i] = static_cast<uint32_t>(a.acc[i]);
    if (a.out_retired_count) a.out_retired_count[i] = a.w.retired_count[i];
  }
  if (i < GZ) {
    const uint64_t run = a.acc[G + i], ret = a.w.retired[i];
    if (a.out_running) a.out_running[i] = run;
    if (a.out_retired) a.out_retired[i] = ret;
    if (a.out_total) a.out_total[i] = run + ret;
  }
}

}  // namespace win
}  // namespace kacc

// =============================================================================
// C ABI
// =============================================================================
struct kacc_window {
  kacc_ctx *ctx = nullptr;  // for errors, the tables and the default stream while the context lives
  int device = 0;           // destroy must not touch ctx (it may be gone already)
  kacc_kind kind = KACC_KIND_PROC;
  uint32_t n_groups = 0, Z = 0;
  uint64_t cap = 0;  // the kind's slot capacity
  uint64_t *d_base = nullptr;
  uint32_t *d_group = nullptr;
  uint64_t *d_retired = nullptr;
  uint32_t *d_rcount = nullptr;
  uint32_t merge_rounds = 0;  // the retire phase's wave merges: kMergeRounds, or the benchmark's knob (read at create)
};

namespace {

kacc::win::State window_state(const kacc_window *w) {
  const kacc_ctx *ctx = w->ctx;
  kacc::win::State s{};
  s.base = w->d_base;
  s.slot_group = w->d_group;
  s.retired = w->d_retired;
  s.retired_count = w->d_rcount;
  s.tab_e = static_cast<const uint64_t *>(ctx->tables[kacc::kind_energy_table(w->kind)]);
  s.tab_stride = w->kind == KACC_KIND_POD ? 2 * w->Z : w->Z;
  s.Z = w->Z;
  s.n_groups = w->n_groups;
  s.cap = w->cap;
  s.err = ctx->d_err;
  return s;
}

// The window's view of the caller's rows: the shared resolver's, without the derived power's
// guard operands (a window reads energy only).
int window_rows(kacc_window *w, const char *fn, const kacc_top_rows *rows, const uint32_t *node_mask,
                kacc::rows::View *v) {
  const int rc = kacc::rows::resolve(w->ctx, fn, w->kind, rows, node_mask, v);
  if (rc == KACC_OK) v->derived = 0;
  return rc;
}

}  // namespace

extern "C" {

int kacc_window_create(kacc_ctx *ctx, kacc_kind kind, uint32_t n_groups, kacc_window **out) {
  const char *fn = "kacc_window_create";
  if (!ctx || !out) return KACC_EINVAL;
  *out = nullptr;
  int rc = kacc::rows::resolve_kind(ctx, fn, kind);
  if (rc != KACC_OK) return rc;
  if ((rc = kacc::rows::check_groups(ctx, fn, n_groups)) != KACC_OK) return rc;
  KACC_HIP(ctx, hipSetDevice(ctx->device));
  auto *w = new kacc_window;
  w->ctx = ctx;
  w->device = ctx->device;
  w->kind = kind;
  w->n_groups = n_groups;
  w->Z = ctx->cfg.zones;
  // a knob of tools/bench_window.py
  w->merge_rounds = kacc::rows::knob("KACC_WINDOW_MERGE_ROUNDS", kacc::win::kMergeRounds, 64u);
  w->cap = kacc::kind_cap(ctx, kind);
  // slots x (base 8Z + id 4): refuse before the allocation when it cannot fit, with the cost in
  // the message (the groups' accumulators are at most 2.3 MB)
  const size_t Z = w->Z, S = static_cast<size_t>(w->cap), per = 8 * Z + 4;
  const size_t need = S * per;
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && need > free_b) {
    delete w;
    return kacc_fail(ctx, KACC_ENOMEM, "window needs %zu B = %zu slots x %zu B, %zu B of device memory free", need, S,
                     per, free_b);
  }
  hipError_t e = hipSuccess;
  auto A = [&](void **p, size_t bytes) {
    if (e == hipSuccess) e = hipMalloc(p, std::max<size_t>(bytes, 16));
  };
  A(reinterpret_cast<void **>(&w->d_base), 8 * S * Z);
  A(reinterpret_cast<void **>(&w->d_group), 4 * S);
  A(reinterpret_cast<void **>(&w->d_retired), 8 * static_cast<size_t>(n_groups) * Z);
  A(reinterpret_cast<void **>(&w->d_rcount), 4 * static_cast<size_t>(n_groups));
  if (e == hipSuccess) e = hipMemsetAsync(w->d_base, 0, std::max<size_t>(8 * S * Z, 16), ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(w->d_group, 0xff, std::max<size_t>(4 * S, 16), ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(w->d_retired, 0, 8 * static_cast<size_t>(n_groups) * Z, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(w->d_rcount, 0, 4 * static_cast<size_t>(n_groups), ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    kacc_window_destroy(w);
    return kacc_fail(ctx, e == hipErrorOutOfMemory ? KACC_ENOMEM : KACC_EHIP,
                     "window allocation (%zu B = %zu slots x %zu B): %s", need, S, per, hipGetErrorString(e));
  }
  *out = w;
  return KACC_OK;
}

void kacc_window_destroy(kacc_window *w) {
  if (!w) return;
  (void)hipSetDevice(w->device);
  (void)hipDeviceSynchronize();  // no launch on this window may still be running
  (void)hipFree(w->d_base);
  (void)hipFree(w->d_group);
  (void)hipFree(w->d_retired);
  (void)hipFree(w->d_rcount);
  delete w;
}

int kacc_window_step(kacc_window *w, const kacc_top_rows *rows, const uint32_t *group, uint32_t flags,
                     const kacc_slotmap *m, const uint32_t *term_slot, const uint32_t *term_count, void *stream) {
  using namespace kacc::win;
  const char *fn = "kacc_window_step";
  if (!w) return KACC_EINVAL;
  kacc_ctx *ctx = w->ctx;
  AdoptArgs a{};
  int rc = window_rows(w, fn, rows, nullptr, &a.v);
  if (rc != KACC_OK) return rc;
  if (!group && w->n_groups != 1)
    return kacc_fail(ctx, KACC_EINVAL, "%s: NULL group with n_groups %u != 1", fn, w->n_groups);
  if (flags & ~KACC_WINDOW_ASSIGN_ALL) return kacc_fail(ctx, KACC_EINVAL, "%s: unknown flags 0x%x", fn, flags);
  if (term_count && (!m || !term_slot))
    return kacc_fail(ctx, KACC_EINVAL, "%s: term_count without a slot map or term_slot", fn);
  if (m && (m->ctx != ctx || m->kind != w->kind))
    return kacc_fail(ctx, KACC_EINVAL, "%s: window and slot map differ in context or kind", fn);
  kacc::rows::Call call(ctx, fn);
  if ((rc = call.open(stream)) != KACC_OK) return rc;
  hipStream_t st = call.st;
  a.w = window_state(w);
  a.group = group;
  a.assign_all = flags & KACC_WINDOW_ASSIGN_ALL;
  const uint32_t tiles = a.v.n_nodes ? kacc::rows::tiles_of(a.v.n_rows, kAdoptTile) : 0u;  // without a node no row is listed
  kacc::plan::Layout tmp;
  if (tiles) tmp.add(&a.v.nflags, a.v.n_nodes);
  if ((rc = call.alloc(tmp)) != KACC_OK) return rc;
  if (term_count && m->n_nodes) {  // (a) before (b): stream order
    RetireArgs r{a.w, m->n_nodes, m->d_slot_off, term_slot, term_count, w->merge_rounds};
    const uint32_t wgs = (m->n_nodes + kRetireWaves - 1) / kRetireWaves;  // one node per wave
    if (static_cast<uint64_t>(w->n_groups) * (1u + w->Z) <= kBigWords)
      KACC_LAUNCH(retire_kernel<true>, dim3(std::min(wgs, kRetireGrid)), dim3(kRetireThreads), 0, st, r);
    else
      KACC_LAUNCH(retire_kernel<false>, dim3(wgs), dim3(kRetireThreads), 0, st, r);
  }
  if (tiles) {
    kacc::rows::launch_node_prep<kThreads>(a.v, a.w.err, kErrGroup, nullptr, st);
    KACC_LAUNCH(adopt_kernel, dim3(tiles), dim3(kThreads), 0, st, a);
  }
  return call.finish();
}

int kacc_window_mark(kacc_window *w, void *stream) {
  using namespace kacc::win;
  const char *fn = "kacc_window_mark";
  if (!w) return KACC_EINVAL;
  kacc_ctx *ctx = w->ctx;
  kacc::rows::Call call(ctx, fn);
  if (const int rc = call.open(stream)) return rc;
  hipStream_t st = call.st;
  const State s = window_state(w);
  KACC_HIP(ctx, hipMemsetAsync(w->d_retired, 0, 8 * static_cast<size_t>(w->n_groups) * w->Z, st));
  KACC_HIP(ctx, hipMemsetAsync(w->d_rcount, 0, 4 * static_cast<size_t>(w->n_groups), st));
  const uint64_t words = w->cap * w->Z;
  if (!words) return KACC_OK;
  const bool vec = s.tab_stride == s.Z && s.Z % 2 == 0;
  const uint64_t n = vec ? words / 2 : words;
  const uint32_t grid = static_cast<uint32_t>(std::min<uint64_t>((n + kThreads - 1) / kThreads, kCus * 32ull));
  if (vec)
    KACC_LAUNCH(mark_kernel<true>, dim3(grid), dim3(kThreads), 0, st, s, n);
  else
    KACC_LAUNCH(mark_kernel<false>, dim3(grid), dim3(kThreads), 0, st, s, n);
  return call.finish();
}

int kacc_window_read(kacc_window *w, const kacc_top_rows *rows, const uint32_t *node_mask, uint32_t *out_count,
                     uint64_t *out_running, uint64_t *out_retired, uint32_t *out_retired_count, uint64_t *out_total,
                     uint64_t *out_row, void *stream) {
  using namespace kacc::win;
  const char *fn = "kacc_window_read";
  if (!w) return KACC_EINVAL;
  kacc_ctx *ctx = w->ctx;
  ReadArgs a{};
  int rc = window_rows(w, fn, rows, node_mask, &a.v);
  if (rc != KACC_OK) return rc;
  if (!out_count && !out_running && !out_retired && !out_retired_count && !out_total && !out_row)
    return kacc_fail(ctx, KACC_EINVAL, "%s: no output array", fn);
  kacc::rows::Call call(ctx, fn);
  if ((rc = call.open(stream)) != KACC_OK) return rc;
  hipStream_t st = call.st;
  a.w = window_state(w);
  const uint32_t Z = a.w.Z, G = a.w.n_groups, W = 1u + Z;
  a.tiles = a.v.n_nodes ? kacc::rows::tiles_of(a.v.n_rows, kReadTile) : 0u;  // without a node no row is listed
  a.out_count = out_count;
  a.out_running = out_running;
  a.out_retired = out_retired;
  a.out_retired_count = out_retired_count;
  a.out_total = out_total;
  a.out_row = out_row;

  // the bins: replicated while they fit the small LDS size, else one copy in the large one, else
  // the accumulator itself
  const kacc::plan::Bins b = kacc::plan::window_bins(G, Z);
  a.copies = b.copies;
  a.copy_stride = b.regime == kacc::plan::kSmall ? (G * W) | 1u : G * W;  // odd: the copies of a bin fall into different banks
  a.splits = kacc::plan::plan_splits(b, a.tiles, 0u);

  // temporaries, stream ordered: the accumulator and the node flags
  kacc::plan::Layout tmp;
  tmp.add(&a.acc, static_cast<uint64_t>(G) * W, true);
  tmp.add(&a.v.nflags, a.v.n_nodes);
  if ((rc = call.alloc(tmp)) != KACC_OK) return rc;
  // rows of a batch without a node: no tile writes them
  if (out_row && !a.tiles && a.v.n_rows && hipMemsetAsync(out_row, 0, 8ull * a.v.n_rows * Z, st) != hipSuccess)
    return kacc_fail(ctx, KACC_EHIP, "%s: memset", fn);

  const dim3 block(kThreads), grid(a.splits);
  if (a.tiles) {
    kacc::rows::launch_node_prep<kThreads>(a.v, a.w.err, kErrGroup, nullptr, st);
    kacc::rows::dispatch_zones(Z, [&](auto z) {
      if (b.regime == kacc::plan::kSmall)
        KACC_LAUNCH((read_kernel<z(), kSmallWords>), grid, block, 0, st, a);
      else if (b.regime == kacc::plan::kBig)
        KACC_LAUNCH((read_kernel<z(), kBigWords>), grid, block, 0, st, a);
      else
        KACC_LAUNCH((read_kernel<z(), 0>), grid, block, 0, st, a);
    });
  }
  const uint64_t words = static_cast<uint64_t>(G) * Z;
  KACC_LAUNCH(finish_kernel, dim3(static_cast<uint32_t>((words + kThreads - 1) / kThreads)), block, 0, st, a);
  return call.finish();
}

int kacc_window_download(kacc_window *w, uint64_t first, uint64_t count, uint64_t *host_base, uint32_t *host_group) {
  if (!w) return KACC_EINVAL;
  kacc_ctx *ctx = w->ctx;
  if (first > w->cap || count > w->cap - first)
    return kacc_fail(ctx, KACC_EINVAL, "window download: range past %llu slots", (unsigned long long)w->cap);
  if (!count || (!host_base && !host_group)) return KACC_OK;
  KACC_HIP(ctx, hipSetDevice(ctx->device));
  KACC_HIP(ctx, hipDeviceSynchronize());  // steps may run on any stream
  if (host_base)
    KACC_HIP(ctx, hipMemcpy(host_base, w->d_base + first * w->Z, 8 * count * w->Z, hipMemcpyDeviceToHost));
  if (host_group) KACC_HIP(ctx, hipMemcpy(host_group, w->d_group + first, 4 * count, hipMemcpyDeviceToHost));
  return KACC_OK;
}

}  // extern "C"
