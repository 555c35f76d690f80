// Value histograms of the running workloads by a caller-defined group, on the device
// (DESIGN §4.14).
//
// No reference counterpart: Kepler exports every running workload and leaves the histogram
// (`_bucket{le=...}`, `_sum`, `_count`) to the consumer.  Row r of the caller's last interval
// batch (one workload kind) has one value - the element of the table at (its slot, zone) - and
// falls in bin j = the number of bounds whose key is below the value's key, of group[r].  Every
// output is an integer count or an integer sum mod 2^64, so the order of the additions is free
// and the result is the same bits for any tiling, any shard split and any number of GPUs.
//
// A group's counters are C = n_bounds + 3 u32 words - the n_bounds + 1 bins, `nan`, `unsummed` -
// plus one u64 sum word.
//
//   node_prep   one thread per node: the listed flag and the guard bit of each zone, ONCE per
//               node (kacc_rows.hpp; kacc_select.hip's)
//   bin         the groups' counters and sums fit in LDS: persistent workgroups, each walks every
//               splits-th tile of kTile batch rows (the row's node by search in row_off), loads
//               every row's value, counts the bounds below it (a compare-and-add loop over the
//               bounds' keys, which are kernel arguments: uniform registers) and adds 1 to the
//               bin with one 32-bit LDS add, and the row's sum word with one 64-bit LDS add
//               unless it is zero.  While they fit more than once the counters are replicated
//               per lane subset with an odd stride, so the lanes of a wave do not queue on one
//               counter
//   rows, pass  more counters than LDS holds: `rows` classifies every row ONCE (one workgroup per
//               tile) into a 4-byte row word - the group id, the counter index within the group,
//               "unsummed" and "has a sum word" bits, or "none" - and the row's 8-byte sum word.
//               `pass` is a grid of passes x splits persistent workgroups; a pass owns a
//               contiguous range of `bins` groups, that is of counters.  Every workgroup reads
//               the tile's row words; only the workgroup whose pass owns the row's group adds
//               it, and only that one loads a non-zero sum word
//   flush       (the end of bin and pass) a workgroup adds its non-zero LDS words into the zeroed
//               u64 accumulator with atomics, consecutive lanes on consecutive words: one atomic
//               per workgroup and word, never one per row
//   finish      one thread per bin: the outputs, out_cum as the prefix over the group's bins
// Every index is clamped (rows to the batch, slots to slot 0, nodes by the search's range, group
// ids and counter indices by the pass's range), so no batch faults.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kacc_derive.hpp"
#include "kacc_internal.hpp"
#include "kacc_rows.hpp"

namespace kacc {
namespace hist {

constexpr uint32_t kThreads = 512;                // 8 waves: three workgroups are 24 waves per CU
constexpr uint32_t kBigThreads = 1024;            // the large LDS size: ONE workgroup of 16 waves per CU, so
                                                  // half as many workgroups flush their counters
constexpr uint32_t kPer = 8;                      // rows per lane and tile, all in flight together
constexpr uint32_t kTile = kThreads * kPer;       // rows per tile (kBigThreads * kPer in the large size)
// LDS sizes in u32 words; a group takes n_bounds + 5 of them
constexpr uint32_t kSmallWords = 8192;            // 32 KiB, three workgroups per CU: replicated counters
constexpr uint32_t kBigWords = 20096;             // 78.5 KiB: 1,004 groups at 15 bounds
constexpr uint32_t kPassWords = 19200;            // a pass's counters: 75 KiB, 960 groups at 15 bounds
constexpr uint32_t kQueue = 128;                  // a wave's queued rows in a pass (4 KiB per workgroup)
constexpr uint32_t kPassPer = 16;                 // row words per lane and step of a pass
constexpr uint32_t kPassTile = kThreads * kPassPer;
constexpr uint32_t kCus = 256;                    // MI355X
constexpr uint32_t kMaxCopies = 64;               // one copy of the counters per lane of a wave
constexpr uint32_t kErrHist = 1u << 14;           // a group id or a slot past its range, a row range
                                                  // outside the batch
constexpr uint64_t kFxLimit = (1023ull + 50ull) << 52;  // the bits of 2^50: |p| at or past it adds no sum
// the row word of the `rows` pass: the group id, the counter index within the group above it
// (a bin, or n_bounds + 1 = `nan`), then the two flags
constexpr uint32_t kWordGroup = 0xffffu, kWordIdxShift = 16, kWordIdx = 0x7fu;
constexpr uint32_t kWordUnsummed = 1u << 23, kWordSum = 1u << 24, kWordNone = 0xffffffffu;
static_assert(KACC_GROUP_MAX <= kWordGroup + 1u && KACC_HIST_MAX_BOUNDS + 2u <= kWordIdx,
              "a row word holds the group id and the counter index");
using rows::kListed;

enum Src { kEnergy = 0, kStored = 1, kDerived = 2 };  // the table of the values

struct Args {
  // the values' table
  const uint64_t *words;  // energy / stored power words of `zone`: words[slot * stride]
  uint32_t stride;        // Z, or 2Z for the pod records
  ProcDerive pd;          // derived power
  uint32_t zone, Z, derived;
  uint64_t cap;  // the kind's slot capacity
  // the bounds
  uint32_t n_bounds;
  uint64_t key[KACC_HIST_MAX_BOUNDS];  // strictly ascending
  // the rows
  uint32_t n_nodes, n_rows, tiles;
  const uint32_t *row_off, *slot, *node_status, *node_mask, *group;  // group NULL: every row in group 0
  uint32_t n_groups;
  // the grid
  uint32_t splits;                        // workgroups that share the tiles
  uint32_t copies, cnt_stride, sum_stride;  // bin: 2^k copies; a copy's counters (u32) and sums (u64) apart
  uint32_t bins, passes;                  // pass: groups per pass; workgroup b takes pass b % passes, split b / passes
  // scratch
  uint32_t *nflags;   // [n_nodes]
  uint64_t *acc;      // [n_groups * C] the counters, [n_groups] the sums
  uint32_t *row_word; // [n_rows] (pass only)
  uint64_t *row_fx;   // [n_rows] (pass only)
  // the outputs
  uint64_t *out_bin, *out_cum, *out_sum, *out_nan, *out_unsummed;
  uint32_t *err;
};

// The order rule's key of a power (header; kacc_top.hip's): NaN lowest, the zeros equal, else
// the IEEE order.
__host__ __device__ __forceinline__ uint64_t power_key(uint64_t b) {
  const uint32_t hi = static_cast<uint32_t>(b >> 32), lo = static_cast<uint32_t>(b);
  const uint32_t mag = hi & 0x7fffffffu;
  if (mag > 0x7ff00000u || (mag == 0x7ff00000u && lo != 0)) return 0;  // NaN
  if ((mag | lo) == 0) return 0x8000000000000000ull;                   // ±0
  return (hi >> 31) ? ~b : (b | 0x8000000000000000ull);
}
// fx(p) of the header (kacc_group.hip's) for the f64 with these bits; keep: it adds to the sum.
__device__ __forceinline__ uint64_t power_fx(uint64_t bits, bool &keep) {
  keep = (bits & 0x7fffffffffffffffull) < kFxLimit;  // finite and |p| < 2^50
  const double p = __longlong_as_double(static_cast<long long>(keep ? bits : 0ull));
  return static_cast<uint64_t>(static_cast<long long>(p * 4096.0));  // exact product, truncated toward zero
}
__device__ __forceinline__ void lds_add(uint64_t *p, uint64_t v) {
  atomicAdd(reinterpret_cast<unsigned long long *>(p), static_cast<unsigned long long>(v));
}

__global__ __launch_bounds__(kThreads) void node_prep_kernel(const Args a) {
  const uint32_t n = blockIdx.x * kThreads + threadIdx.x;
  if (n >= a.n_nodes) return;
  bool bad_range;
  const uint32_t f = rows::node_flags(a.row_off, a.node_status, a.node_mask, a.pd, a.derived, a.Z, a.n_rows, n, bad_range);
  if (bad_range) atomicOr(a.err, kErrHist);  // left out
  a.nflags[n] = f;
}

struct TileRows {  // a lane's kPer rows of a tile
  bool in_batch[kPer], ok[kPer], uns[kPer];  // ok: the row contributes; uns: binned, but no sum word
  uint32_t r[kPer], g[kPer], idx[kPer];      // idx: the counter within the group (a bin, or `nan`)
  uint64_t fx[kPer];                         // the sum word
};
// Classifies the tile's rows and evaluates them; true when a listed row of this lane has a slot
// or a group id out of range.  No load sits behind a data-dependent branch: a row past the
// batch is clamped to its last row, a bad slot to slot 0.
template <int kSrc, uint32_t kT>  // kT: the workgroup's threads, a tile is kT * kPer rows
__device__ __forceinline__ bool classify_tile(const Args &a, uint32_t tile, uint32_t lane, uint32_t wave, TileRows &t) {
  const rows::TileNodes tn = rows::tile_nodes(a.row_off, a.n_nodes, a.n_rows, tile, kT * kPer, lane);
  const uint64_t row0 = static_cast<uint64_t>(tile) * (kT * kPer) + wave * (kPer * 64u) + lane;
  const uint32_t last_row = a.n_rows - 1;
  uint32_t w[kPer], node[kPer], hi[kPer];
#pragma unroll
  for (uint32_t u = 0; u < kPer; ++u) {
    const uint64_t rr = row0 + u * 64u;
    t.in_batch[u] = rr <= last_row;
    t.r[u] = static_cast<uint32_t>(min(rr, static_cast<uint64_t>(last_row)));
    w[u] = a.slot[t.r[u]];
    t.g[u] = a.group ? a.group[t.r[u]] : 0u;  // uniform
    node[u] = tn.first;
    hi[u] = tn.last;
  }
  for (uint32_t s = 0; s < tn.steps; ++s) {  // workgroup-uniform
#pragma unroll
    for (uint32_t u = 0; u < kPer; ++u) rows::node_step(a.row_off, t.r[u], node[u], hi[u]);
  }
  bool bad = false;
  uint64_t v[kPer], key[kPer];
#pragma unroll
  for (uint32_t u = 0; u < kPer; ++u) {
    const uint32_t n = node[u];
    const uint32_t r0 = a.row_off[n], r1 = a.row_off[n + 1];
    const uint32_t f = a.nflags[n];
    const bool listed = t.in_batch[u] && r0 <= t.r[u] && t.r[u] < r1 && (f & kListed);
    const uint32_t s = w[u] & KACC_SLOT_MASK;
    const bool in = s < a.cap, gin = t.g[u] < a.n_groups;
    bad = bad || (listed && (!in || (!gin && t.g[u] != KACC_GROUP_NONE)));  // left out
    t.ok[u] = listed && in && gin;
    const uint64_t sl = in ? s : 0u;
    v[u] = 0;
    if (a.cap != 0) {  // uniform
      if constexpr (kSrc == kDerived) {
        const double ratio = a.pd.ratio[sl];
        const double aP = a.pd.active_power[static_cast<uint64_t>(n) * a.Z + a.zone];
        v[u] = static_cast<uint64_t>(__double_as_longlong(((f >> a.zone) & 1u) ? ratio * aP : 0.0));
      } else {
        v[u] = a.words[sl * a.stride];
      }
    }
    key[u] = kSrc == kEnergy ? v[u] : power_key(v[u]);
    t.idx[u] = 0;
  }
  for (uint32_t i = 0; i < a.n_bounds; ++i) {  // uniform: the bound's key is a scalar
    const uint64_t kb = a.key[i];
#pragma unroll
    for (uint32_t u = 0; u < kPer; ++u) t.idx[u] += kb < key[u];
  }
#pragma unroll
  for (uint32_t u = 0; u < kPer; ++u) {
    if constexpr (kSrc == kEnergy) {
      t.fx[u] = v[u];
      t.uns[u] = false;
    } else {
      bool keep;
      t.fx[u] = power_fx(v[u], keep);
      const bool nan = key[u] == 0;  // only a NaN has key 0
      t.idx[u] = nan ? a.n_bounds + 1u : t.idx[u];
      t.uns[u] = !keep && !nan;
    }
  }
  return bad;
}

// The flush: the workgroup's counters and sums of groups [g0, g0 + nloc) (the copies summed)
// into the accumulator, consecutive lanes on consecutive words.
__device__ __forceinline__ void flush_bins(const Args &a, const uint32_t *s_cnt, uint32_t cnt_stride,
                                           const uint64_t *s_sum, uint32_t sum_stride, uint32_t copies, uint32_t g0,
                                           uint32_t nloc, uint32_t tid, uint32_t threads) {
  const uint32_t C = a.n_bounds + 3u;
  for (uint32_t i = tid; i < nloc * C; i += threads) {
    uint64_t v = 0;
    for (uint32_t c = 0; c < copies; ++c) v += s_cnt[c * cnt_stride + i];
    if (v == 0) continue;
    atomicAdd(reinterpret_cast<unsigned long long *>(a.acc + static_cast<uint64_t>(g0) * C + i),
              static_cast<unsigned long long>(v));
  }
  for (uint32_t i = tid; i < nloc; i += threads) {
    uint64_t v = 0;
    for (uint32_t c = 0; c < copies; ++c) v += s_sum[c * sum_stride + i];
    if (v == 0) continue;
    atomicAdd(reinterpret_cast<unsigned long long *>(a.acc + static_cast<uint64_t>(a.n_groups) * C + g0 + i),
              static_cast<unsigned long long>(v));
  }
}

// Every group's counters and sums in LDS, `copies` times: the sums of all copies first (u64),
// the counters behind them.
template <int kSrc, uint32_t kLds>
__global__ __launch_bounds__(kLds == kSmallWords ? kThreads : kBigThreads, kLds == kSmallWords ? 6 : 4) void bin_kernel(
    const Args a) {
  constexpr uint32_t kT = kLds == kSmallWords ? kThreads : kBigThreads;
  __shared__ uint64_t s_mem[kLds / 2];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t C = a.n_bounds + 3u;
  uint32_t *const s32 = reinterpret_cast<uint32_t *>(s_mem);
  const uint32_t cnt0 = 2u * a.copies * a.sum_stride;                  // the counters' first word
  for (uint32_t i = tid; i < cnt0 + a.copies * a.cnt_stride; i += kT) s32[i] = 0;  // <= kLds (host)
  __syncthreads();
  const uint32_t copy = lane & (a.copies - 1u);
  uint64_t *const b_sum = s_mem + copy * a.sum_stride;
  uint32_t *const b_cnt = s32 + cnt0 + copy * a.cnt_stride;
  bool bad = false;
  for (uint32_t tile = blockIdx.x; tile < a.tiles; tile += a.splits) {  // workgroup-uniform
    TileRows t;
    bad = classify_tile<kSrc, kT>(a, tile, lane, wave, t) || bad;
#pragma unroll
    for (uint32_t u = 0; u < kPer; ++u) {
      if (!t.ok[u]) continue;
      uint32_t *const c = b_cnt + t.g[u] * C;
      atomicAdd(c + t.idx[u], 1u);
      if (t.fx[u]) lds_add(b_sum + t.g[u], t.fx[u]);
      if (t.uns[u]) atomicAdd(c + a.n_bounds + 2u, 1u);
    }
  }
  if (bad) atomicOr(a.err, kErrHist);
  __syncthreads();
  flush_bins(a, s32 + cnt0, a.cnt_stride, s_mem, a.sum_stride, a.copies, 0u, a.n_groups, tid, kT);
}

// One workgroup per tile: the row word (group id | counter index << 16 | flags, or kWordNone for
// a row that does not contribute) and the sum word of every row of the batch.
template <int kSrc>
__global__ __launch_bounds__(kThreads) void rows_kernel(const Args a) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  TileRows t;
  if (classify_tile<kSrc, kThreads>(a, blockIdx.x, lane, wave, t)) atomicOr(a.err, kErrHist);
#pragma unroll
  for (uint32_t u = 0; u < kPer; ++u) {
    if (!t.in_batch[u]) continue;
    const uint32_t word = t.g[u] | t.idx[u] << kWordIdxShift | (t.uns[u] ? kWordUnsummed : 0u) | (t.fx[u] ? kWordSum : 0u);
    a.row_word[t.r[u]] = t.ok[u] ? word : kWordNone;
    a.row_fx[t.r[u]] = t.fx[u];
  }
}

__device__ __forceinline__ void wave_lds_fence() {  // a wave's LDS writes before its reads (kacc_select.hip's)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// A pass's range of groups in LDS; the rows by their row words.  About one row word in `passes`
// is the pass's, so a wave first queues its rows (ballot and popcount, in LDS) and adds 64
// queued rows at a time, one per lane: the sum words' loads of 64 rows are in flight together.
__global__ __launch_bounds__(kThreads, 4) void pass_kernel(const Args a) {
  __shared__ uint64_t s_mem[kPassWords / 2];
  __shared__ uint32_t s_q[kThreads / 64][kQueue];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t C = a.n_bounds + 3u;
  const uint32_t pass = blockIdx.x % a.passes, split = blockIdx.x / a.passes;
  const uint32_t g0 = pass * a.bins;  // < n_groups
  const uint32_t nloc = min(a.bins, a.n_groups - g0);
  uint32_t *const s32 = reinterpret_cast<uint32_t *>(s_mem);
  for (uint32_t i = tid; i < nloc * (C + 2u); i += kThreads) s32[i] = 0;  // <= kPassWords (host)
  __syncthreads();
  uint64_t *const b_sum = s_mem;
  uint32_t *const b_cnt = s32 + 2u * nloc;
  uint32_t *const q = s_q[wave];
  const uint32_t last_row = a.n_rows - 1;
  const uint32_t pass_tiles = static_cast<uint32_t>((static_cast<uint64_t>(a.n_rows) + kPassTile - 1) / kPassTile);

  // the queued rows q[0 .. n) of this wave, n <= 64, one per lane
  auto drain = [&](uint32_t n) {
    if (lane >= n) return;
    const uint32_t r = min(q[lane], last_row);
    const uint32_t word = a.row_word[r];
    const uint32_t g = min((word & kWordGroup) - g0, nloc - 1u);  // the pass's: checked when it was queued
    const uint32_t idx = min((word >> kWordIdxShift) & kWordIdx, a.n_bounds + 1u);
    uint32_t *const c = b_cnt + g * C;
    atomicAdd(c + idx, 1u);
    if (word & kWordSum) lds_add(b_sum + g, a.row_fx[r]);
    if (word & kWordUnsummed) atomicAdd(c + a.n_bounds + 2u, 1u);
  };

  uint32_t qn = 0;  // wave-uniform: the queued rows, < 64 between steps
  for (uint32_t tile = split; tile < pass_tiles; tile += a.splits) {  // workgroup-uniform
    const uint64_t row0 = static_cast<uint64_t>(tile) * kPassTile + wave * (kPassPer * 64u) + lane;
    uint32_t word[kPassPer];
#pragma unroll
    for (uint32_t u = 0; u < kPassPer; ++u)  // a row past the batch is clamped to its last row
      word[u] = a.row_word[static_cast<uint32_t>(min(row0 + u * 64u, static_cast<uint64_t>(last_row)))];
#pragma unroll
    for (uint32_t u = 0; u < kPassPer; ++u) {
      const uint64_t rr = row0 + u * 64u;
      const bool mine = rr <= last_row && word[u] != kWordNone && (word[u] & kWordGroup) - g0 < nloc;
      const uint64_t m = __ballot(mine);
      if (m == 0) continue;  // wave-uniform
      if (mine) q[qn + static_cast<uint32_t>(__popcll(m & ((1ull << lane) - 1ull)))] = static_cast<uint32_t>(rr);
      qn += static_cast<uint32_t>(__popcll(m));  // <= 127 < kQueue
      if (qn >= 64u) {
        wave_lds_fence();
        drain(64u);
        const uint32_t rest = qn - 64u;  // < 64
        const uint32_t moved = q[64u + min(lane, 63u)];
        wave_lds_fence();
        if (lane < rest) q[lane] = moved;
        qn = rest;
      }
    }
  }
  wave_lds_fence();
  drain(qn);
  __syncthreads();
  flush_bins(a, b_cnt, 0u, b_sum, 0u, 1u, g0, nloc, tid, kThreads);
}

// Every non-NULL output out of the accumulator: thread i is bin i % B1 of group i / B1, and
// group i's sum, nan and unsummed words.
__global__ __launch_bounds__(kThreads) void finish_kernel(const Args a) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
  const uint64_t G = a.n_groups, B1 = a.n_bounds + 1u, C = B1 + 2u;
  if (i < G) {
    if (a.out_sum) a.out_sum[i] = a.acc[G * C + i];
    if (a.out_nan) a.out_nan[i] = a.acc[i * C + B1];
    if (a.out_unsummed) a.out_unsummed[i] = a.acc[i * C + B1 + 1u];
  }
  if (i < G * B1) {
    const uint64_t g = i / B1, j = i - g * B1;
    const uint64_t *c = a.acc + g * C;
    if (a.out_bin) a.out_bin[i] = c[j];
    if (a.out_cum) {
      uint64_t s = 0;
      for (uint64_t k = 0; k <= j; ++k) s += c[k];
      a.out_cum[i] = s;
    }
  }
}

}  // namespace hist
}  // namespace kacc

namespace {

// The table's kind, or -1 when t is not one of the eight workload tables.
int table_kind(int t) {
  switch (t) {
    case KACC_T_PROC_ENERGY: case KACC_T_PROC_POWER: return KACC_KIND_PROC;
    case KACC_T_CTR_ENERGY: case KACC_T_CTR_POWER: return KACC_KIND_CTR;
    case KACC_T_VM_ENERGY: case KACC_T_VM_POWER: return KACC_KIND_VM;
    case KACC_T_POD_ENERGY: case KACC_T_POD_POWER: return KACC_KIND_POD;
    default: return -1;
  }
}

}  // namespace

extern "C" {

int kacc_group_hist(kacc_ctx *ctx, kacc_table t, uint32_t zone, const kacc_top_rows *rows, const uint32_t *group,
                    uint32_t n_groups, const uint64_t *bounds, uint32_t n_bounds, const uint32_t *node_mask,
                    uint64_t *out_bin, uint64_t *out_cum, uint64_t *out_sum, uint64_t *out_nan,
                    uint64_t *out_unsummed, void *stream) {
  using namespace kacc::hist;
  const char *fn = "kacc_group_hist";
  if (!ctx) return KACC_EINVAL;
  const int kind = table_kind(t);
  if (kind < 0) return kacc_fail(ctx, KACC_EINVAL, "%s: table %d is not a workload energy / power table", fn, (int)t);
  const uint32_t Z = ctx->cfg.zones;
  if (zone >= Z) return kacc_fail(ctx, KACC_EINVAL, "%s: zone %u >= Z = %u", fn, zone, Z);
  if (!rows || !bounds) return kacc_fail(ctx, KACC_EINVAL, "%s: NULL argument", fn);
  if (n_bounds < 1 || n_bounds > KACC_HIST_MAX_BOUNDS)
    return kacc_fail(ctx, KACC_EINVAL, "%s: n_bounds %u outside 1 .. %u", fn, n_bounds, KACC_HIST_MAX_BOUNDS);
  if (n_groups < 1 || n_groups > KACC_GROUP_MAX)
    return kacc_fail(ctx, KACC_EINVAL, "%s: n_groups %u outside 1 .. %u", fn, n_groups, KACC_GROUP_MAX);
  if (static_cast<uint64_t>(n_groups) * (n_bounds + 1u) > KACC_HIST_MAX_BINS)
    return kacc_fail(ctx, KACC_EINVAL, "%s: %u groups x %u bins > %u", fn, n_groups, n_bounds + 1u, KACC_HIST_MAX_BINS);
  if (!group && n_groups != 1) return kacc_fail(ctx, KACC_EINVAL, "%s: NULL group with n_groups %u", fn, n_groups);
  if (rows->n_nodes > ctx->cfg.nodes)
    return kacc_fail(ctx, KACC_EINVAL, "%s: n_nodes %u > the context's %llu nodes", fn, rows->n_nodes,
                     (unsigned long long)ctx->cfg.nodes);
  if (!rows->row_off || (rows->n_rows && !rows->slot)) return kacc_fail(ctx, KACC_EINVAL, "%s: NULL row array", fn);
  if (!out_bin && !out_cum && !out_sum && !out_nan && !out_unsummed)
    return kacc_fail(ctx, KACC_EINVAL, "%s: no output array", fn);

  Args a{};
  const bool power = t == KACC_T_PROC_POWER || t == KACC_T_CTR_POWER || t == KACC_T_VM_POWER || t == KACC_T_POD_POWER;
  const bool pod = kind == KACC_KIND_POD;
  for (uint32_t i = 0; i < n_bounds; ++i) {  // the host array is read here, before the call returns
    a.key[i] = power ? power_key(bounds[i]) : bounds[i];
    if (power && a.key[i] == 0) return kacc_fail(ctx, KACC_EINVAL, "%s: bound %u is a NaN", fn, i);
    if (i && a.key[i] <= a.key[i - 1])
      return kacc_fail(ctx, KACC_EINVAL, "%s: the keys of bounds %u and %u are not strictly ascending", fn, i - 1, i);
  }
  KACC_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
  kacc::TimingScope timing(ctx);

  a.cap = kind == KACC_KIND_PROC ? ctx->cfg.proc_slots
          : kind == KACC_KIND_CTR ? ctx->cfg.ctr_slots
          : kind == KACC_KIND_VM ? ctx->cfg.vm_slots
                                 : ctx->cfg.pod_slots;
  a.pd = kacc_derive(ctx, static_cast<kacc_kind>(pod ? KACC_KIND_PROC : kind));
  a.derived = !pod;  // the kind's power: node_prep evaluates the guards for it
  const int src = !power ? kEnergy : pod ? kStored : kDerived;
  a.stride = pod ? 2 * Z : Z;
  a.words = static_cast<const uint64_t *>(ctx->tables[t]) + zone;  // pod power: Z words into the record
  a.zone = zone;
  a.Z = Z;
  a.n_bounds = n_bounds;
  a.n_nodes = rows->n_nodes;
  a.n_rows = rows->n_rows;
  a.row_off = rows->row_off;
  a.slot = rows->slot;
  a.node_status = rows->node_status;
  a.node_mask = node_mask;
  a.group = group;
  a.n_groups = n_groups;
  a.out_bin = out_bin;
  a.out_cum = out_cum;
  a.out_sum = out_sum;
  a.out_nan = out_nan;
  a.out_unsummed = out_unsummed;
  a.err = ctx->d_err;

  // the grid: replicated counters while a copy (odd strides: the copies of a counter fall into
  // different banks) fits the small LDS size, else one copy in the large one, else passes over
  // group ranges
  const uint32_t C = n_bounds + 3u, W = C + 2u;  // u32 words per group: the counters, the u64 sum
  const uint32_t cnt_odd = (n_groups * C) | 1u, sum_odd = n_groups | 1u, per = cnt_odd + 2u * sum_odd;
  uint32_t lds = kBigWords;
  a.copies = 1;
  a.cnt_stride = n_groups * C;
  a.sum_stride = n_groups;
  a.passes = 1;
  a.bins = n_groups;
  if (per <= kSmallWords) {
    lds = kSmallWords;
    a.cnt_stride = cnt_odd;
    a.sum_stride = sum_odd;
    while (a.copies < kMaxCopies && 2 * a.copies * per <= kSmallWords) a.copies *= 2;
  } else if (n_groups * W > kBigWords) {
    a.bins = kPassWords / W;
    a.passes = (n_groups + a.bins - 1) / a.bins;
  }
  // workgroups per CU: three of 512 threads at the small size, one of 1,024 at the large one, two of 512 in a pass
  const bool big = a.passes == 1 && lds == kBigWords;
  const uint32_t wgs = kCus * (lds == kSmallWords ? 3u : big ? 1u : 2u);
  const uint32_t tile_rows = big ? kBigThreads * kPer : kTile;
  // without a node no row is listed
  a.tiles = a.n_nodes ? static_cast<uint32_t>((static_cast<uint64_t>(a.n_rows) + tile_rows - 1) / tile_rows) : 0u;
  const uint32_t pass_tiles = static_cast<uint32_t>((static_cast<uint64_t>(a.n_rows) + kPassTile - 1) / kPassTile);
  a.splits = std::max(1u, a.passes > 1 ? std::min(pass_tiles, wgs / a.passes) : std::min(a.tiles, wgs));

  // temporaries, stream ordered: the accumulator, for passes the sum and row words, the node flags
  const uint64_t acc_words = static_cast<uint64_t>(n_groups) * (C + 1u);
  const uint64_t row_words = a.passes > 1 && a.tiles ? a.n_rows : 0;
  uint64_t *tmp = nullptr;
  KACC_HIP(ctx, hipMallocAsync(reinterpret_cast<void **>(&tmp), 8 * acc_words + 12 * row_words + 4ull * a.n_nodes, st));
  a.acc = tmp;
  a.row_fx = tmp + acc_words;
  a.row_word = reinterpret_cast<uint32_t *>(a.row_fx + row_words);
  a.nflags = a.row_word + row_words;
  int rc = KACC_OK;
  if (hipMemsetAsync(a.acc, 0, 8 * acc_words, st) != hipSuccess) rc = kacc_fail(ctx, KACC_EHIP, "%s: memset", fn);

  if (rc == KACC_OK) {
    (void)hipGetLastError();  // clear a stale error of an earlier call
    const dim3 block(kThreads);
    if (a.n_nodes) KACC_LAUNCH(node_prep_kernel, dim3((a.n_nodes + kThreads - 1) / kThreads), block, 0, st, a);
    if (a.tiles) {
      if (a.passes > 1) {
        if (src == kEnergy)
          KACC_LAUNCH(rows_kernel<kEnergy>, dim3(a.tiles), block, 0, st, a);
        else if (src == kStored)
          KACC_LAUNCH(rows_kernel<kStored>, dim3(a.tiles), block, 0, st, a);
        else
          KACC_LAUNCH(rows_kernel<kDerived>, dim3(a.tiles), block, 0, st, a);
        KACC_LAUNCH(pass_kernel, dim3(a.passes * a.splits), block, 0, st, a);
      } else if (lds == kSmallWords) {
        if (src == kEnergy)
          KACC_LAUNCH((bin_kernel<kEnergy, kSmallWords>), dim3(a.splits), block, 0, st, a);
        else if (src == kStored)
          KACC_LAUNCH((bin_kernel<kStored, kSmallWords>), dim3(a.splits), block, 0, st, a);
        else
          KACC_LAUNCH((bin_kernel<kDerived, kSmallWords>), dim3(a.splits), block, 0, st, a);
      } else {
        const dim3 big_block(kBigThreads);
        if (src == kEnergy)
          KACC_LAUNCH((bin_kernel<kEnergy, kBigWords>), dim3(a.splits), big_block, 0, st, a);
        else if (src == kStored)
          KACC_LAUNCH((bin_kernel<kStored, kBigWords>), dim3(a.splits), big_block, 0, st, a);
        else
          KACC_LAUNCH((bin_kernel<kDerived, kBigWords>), dim3(a.splits), big_block, 0, st, a);
      }
    }
    const uint64_t words = static_cast<uint64_t>(n_groups) * (n_bounds + 1u);
    KACC_LAUNCH(finish_kernel, dim3(static_cast<uint32_t>((words + kThreads - 1) / kThreads)), block, 0, st, a);
    if (hipGetLastError() != hipSuccess) rc = kacc_fail(ctx, KACC_EHIP, "%s: launch", fn);
  }
  (void)hipFreeAsync(tmp, st);
  return rc;
}

}  // extern "C"
