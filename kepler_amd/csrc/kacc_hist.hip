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
// The rows, their values, their nodes' flag words, the tile prelude and the pass queue are the
// shared row layer's (kacc_rows.hpp); this file adds the bounds and the counters on top.
//
//   node_prep   the shared layer's: one flag word per node
//   bin         the groups' counters and sums fit in LDS: persistent workgroups, each walks every
//               splits-th tile of kTile batch rows (located by the shared prelude), loads
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
// Every index is clamped (the shared layer's rules; group ids and counter indices by the
// pass's range), so no batch faults.
#include <hip/hip_runtime.h>

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
static_assert(kSmallWords == plan::kHistLds.small_words && kBigWords == plan::kHistLds.big_words &&
                  kPassWords == plan::kHistLds.pass_words, "the host plans with the kernels' LDS sizes");
constexpr uint32_t kPassTile = kThreads * rows::kPassPer;  // the queues: 4 KiB per workgroup
constexpr uint32_t kErrHist = 1u << 14;           // a group id or a slot past its range, a row range
                                                  // outside the batch
// the row word of the `rows` pass: the group id, the counter index within the group above it
// (a bin, or n_bounds + 1 = `nan`), then the two flags
constexpr uint32_t kWordGroup = 0xffffu, kWordIdxShift = 16, kWordIdx = 0x7fu;
constexpr uint32_t kWordUnsummed = 1u << 23, kWordSum = 1u << 24, kWordNone = 0xffffffffu;
static_assert(KACC_GROUP_MAX <= kWordGroup + 1u && KACC_HIST_MAX_BOUNDS + 2u <= kWordIdx,
              "a row word holds the group id and the counter index");
using rows::kQueue, rows::lds_add;
using rows::kDerived, rows::kEnergy, rows::kStored;  // the table of the values

struct Args {
  rows::View v;
  // the values' table
  const uint64_t *words;  // energy / stored power words of `zone`: words[slot * v.tab_stride]
  uint32_t zone;
  // the bounds
  uint32_t n_bounds;
  uint64_t key[KACC_HIST_MAX_BOUNDS];  // strictly ascending
  const uint32_t *group;  // NULL: every row in group 0
  uint32_t n_groups, tiles;
  // the grid
  uint32_t splits;                        // workgroups that share the tiles
  uint32_t copies, cnt_stride, sum_stride;  // bin: 2^k copies; a copy's counters (u32) and sums (u64) apart
  uint32_t bins, passes;                  // pass: groups per pass; workgroup b takes pass b % passes, split b / passes
  // scratch
  uint64_t *acc;      // [n_groups * C] the counters, [n_groups] the sums
  uint32_t *row_word; // [n_rows] (pass only)
  uint64_t *row_fx;   // [n_rows] (pass only)
  // the outputs
  uint64_t *out_bin, *out_cum, *out_sum, *out_nan, *out_unsummed;
  uint32_t *err;
};

struct TileRows {  // a lane's kPer rows of a tile
  bool in_batch[kPer], ok[kPer], uns[kPer];  // ok: the row contributes; uns: binned, but no sum word
  uint32_t r[kPer], g[kPer], idx[kPer];      // idx: the counter within the group (a bin, or `nan`)
  uint64_t fx[kPer];                         // the sum word
};
// Locates the tile's rows (the shared prelude) and evaluates them; true when a listed row of
// this lane has a slot or a group id out of range.
template <int kSrc, uint32_t kT>  // kT: the workgroup's threads, a tile is kT * kPer rows
__device__ __forceinline__ bool classify_tile(const Args &a, uint32_t tile, uint32_t lane, uint32_t wave, TileRows &t) {
  rows::Located<kPer> l;
  rows::locate<kPer>(a.v, a.group, tile, kT * kPer, lane, wave, l);
  uint64_t v[kPer], key[kPer];
#pragma unroll
  for (uint32_t u = 0; u < kPer; ++u) {
    rows::check_row(a.v, a.n_groups, l, u);
    t.in_batch[u] = l.in_batch[u];
    t.ok[u] = l.ok[u];
    t.r[u] = l.r[u];
    t.g[u] = l.g[u];
    v[u] = 0;
    if (a.v.cap != 0)  // uniform
      v[u] = rows::value_bits<kSrc>(a.words, a.v.tab_stride, a.v.pd, a.v.Z, a.zone, l.sl[u], l.node[u], l.f[u]);
    key[u] = kSrc == kEnergy ? v[u] : rows::power_key(v[u]);
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
      t.fx[u] = rows::power_fx(v[u], keep);
      const bool nan = key[u] == 0;  // only a NaN has key 0
      t.idx[u] = nan ? a.n_bounds + 1u : t.idx[u];
      t.uns[u] = !keep && !nan;
    }
  }
  return l.bad;
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
  const uint32_t last_row = a.v.n_rows - 1;

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

  rows::pass_queue<kThreads>(
      a.row_word, a.v.n_rows, split, a.splits, lane, wave, q,
      [&](uint32_t word) { return word != kWordNone && (word & kWordGroup) - g0 < nloc; }, drain);
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

extern "C" {

int kacc_group_hist(kacc_ctx *ctx, kacc_table t, uint32_t zone, const kacc_top_rows *rows, const uint32_t *group,
                    uint32_t n_groups, const uint64_t *bounds, uint32_t n_bounds, const uint32_t *node_mask,
                    uint64_t *out_bin, uint64_t *out_cum, uint64_t *out_sum, uint64_t *out_nan,
                    uint64_t *out_unsummed, void *stream) {
  using namespace kacc::hist;
  const char *fn = "kacc_group_hist";
  if (!ctx) return KACC_EINVAL;
  kacc::rows::Table tab;
  Args a{};
  int rc = kacc::rows::resolve_table(ctx, fn, t, zone, &tab);
  if (rc != KACC_OK) return rc;
  if (!rows || !bounds) return kacc_fail(ctx, KACC_EINVAL, "%s: NULL argument", fn);
  if (n_bounds < 1 || n_bounds > KACC_HIST_MAX_BOUNDS)
    return kacc_fail(ctx, KACC_EINVAL, "%s: n_bounds %u outside 1 .. %u", fn, n_bounds, KACC_HIST_MAX_BOUNDS);
  if ((rc = kacc::rows::check_groups(ctx, fn, n_groups)) != KACC_OK) return rc;
  if (static_cast<uint64_t>(n_groups) * (n_bounds + 1u) > KACC_HIST_MAX_BINS)
    return kacc_fail(ctx, KACC_EINVAL, "%s: %u groups x %u bins > %u", fn, n_groups, n_bounds + 1u, KACC_HIST_MAX_BINS);
  if (!group && n_groups != 1) return kacc_fail(ctx, KACC_EINVAL, "%s: NULL group with n_groups %u", fn, n_groups);
  if ((rc = kacc::rows::resolve(ctx, fn, tab.kind, rows, node_mask, &a.v)) != KACC_OK) return rc;
  if (!out_bin && !out_cum && !out_sum && !out_nan && !out_unsummed)
    return kacc_fail(ctx, KACC_EINVAL, "%s: no output array", fn);

  const bool power = tab.power;
  for (uint32_t i = 0; i < n_bounds; ++i) {  // the host array is read here, before the call returns
    a.key[i] = power ? kacc::rows::power_key(bounds[i]) : bounds[i];
    if (power && a.key[i] == 0) return kacc_fail(ctx, KACC_EINVAL, "%s: bound %u is a NaN", fn, i);
    if (i && a.key[i] <= a.key[i - 1])
      return kacc_fail(ctx, KACC_EINVAL, "%s: the keys of bounds %u and %u are not strictly ascending", fn, i - 1, i);
  }
  kacc::rows::Call call(ctx, fn);
  if ((rc = call.open(stream)) != KACC_OK) return rc;
  hipStream_t st = call.st;

  a.words = tab.words;
  a.zone = zone;
  a.n_bounds = n_bounds;
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
  // workgroups per CU: three of 512 threads at the small size, one of 1,024 at the large one, two of 512 in a pass
  const uint32_t C = n_bounds + 3u;  // a group's counters; with the u64 sum C + 2 u32 words
  const kacc::plan::Bins b = kacc::plan::hist_bins(n_groups, n_bounds);
  const bool small = b.regime == kacc::plan::kSmall, big = b.regime == kacc::plan::kBig;
  a.copies = b.copies;
  a.cnt_stride = small ? (n_groups * C) | 1u : n_groups * C;
  a.sum_stride = small ? n_groups | 1u : n_groups;
  a.passes = b.passes;
  a.bins = b.bins;
  // without a node no row is listed
  a.tiles = a.v.n_nodes ? kacc::rows::tiles_of(a.v.n_rows, big ? kBigThreads * kPer : kTile) : 0u;
  a.splits = kacc::plan::plan_splits(b, a.tiles, kacc::rows::tiles_of(a.v.n_rows, kPassTile));

  // temporaries, stream ordered: the accumulator, for passes the sum and row words, the node flags
  const uint64_t row_words = a.passes > 1 && a.tiles ? a.v.n_rows : 0;
  kacc::plan::Layout tmp;
  tmp.add(&a.acc, static_cast<uint64_t>(n_groups) * (C + 1u), true);
  tmp.add(&a.row_fx, row_words);
  tmp.add(&a.row_word, row_words);
  tmp.add(&a.v.nflags, a.v.n_nodes);
  if ((rc = call.alloc(tmp)) != KACC_OK) return rc;

  const dim3 block(kThreads);
  if (a.v.n_nodes) kacc::rows::launch_node_prep<kThreads>(a.v, a.err, kErrHist, nullptr, st);
  if (a.tiles) {
    kacc::rows::dispatch_src(tab.src, [&](auto s) {
      if (a.passes > 1) {
        KACC_LAUNCH(rows_kernel<s()>, dim3(a.tiles), block, 0, st, a);
        KACC_LAUNCH(pass_kernel, dim3(a.passes * a.splits), block, 0, st, a);
      } else if (small) {
        KACC_LAUNCH((bin_kernel<s(), kSmallWords>), dim3(a.splits), block, 0, st, a);
      } else {
        KACC_LAUNCH((bin_kernel<s(), kBigWords>), dim3(a.splits), dim3(kBigThreads), 0, st, a);
      }
    });
  }
  const uint64_t words = static_cast<uint64_t>(n_groups) * (n_bounds + 1u);
  KACC_LAUNCH(finish_kernel, dim3(static_cast<uint32_t>((words + kThreads - 1) / kThreads)), block, 0, st, a);
  return call.finish();
}

}  // extern "C"
