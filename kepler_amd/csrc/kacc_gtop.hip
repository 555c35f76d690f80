// Top-K running workloads per caller-defined group, on the device.
//
// No reference counterpart: Kepler exports every running workload and leaves `topk by (label)`
// to the consumer.  Row r of the caller's last interval batch (one workload kind) has one value -
// the element of the table at (its slot, zone) - and is ranked inside group[r] by the top lists'
// order: descending u64 sort key, equal keys in ascending batch row order.  Group g's list is the
// first min(k, n_g) of its rows in that order.  The composite (~key, row) is unique per row, so
// the list is the set of rows at or below ONE threshold composite, found by a radix select -
// eight 8-bit digits of ~key from the top and, only where the cut falls inside a block of equal
// keys, the digits of the row index.  Every step is an integer count or a comparison, and the
// lists are sorted by the unique composite before they leave: the same bytes for any tiling.
//
// The rows, their values, their nodes' flag words and the tile prelude are the shared row
// layer's (kacc_rows.hpp).  The digit counters and the pick have the quantiles' shape
// (kacc_quant.hip) with one query per group; they are this file's own copies.
//
//   node_prep   the shared layer's: one flag word per node
//   keys        one workgroup per tile of kTile batch rows: every row is classified ONCE into
//               ~key (8 bytes: ascending order is list order; a NaN power is all ones, ranked
//               last) and a group word (the id, or kNone for a row that does not contribute).
//               The record index is the batch row; the later passes touch only records
//   digit       (eight times over ~key, then row_passes times over the row index) a row adds 1
//               to bins[group][digit] when it carries the digits decided so far.  While the
//               n_groups * 256 u32 counters fit a workgroup's LDS they live there (replicated
//               per lane subset while they fit more than once); past that the lanes of a wave
//               that hit one word merge into one global add
//   pick        one wave per group: the digit whose cumulative count passes the rank that
//               remains.  It zeroes the counters it has read.  The first pick learns n_g and
//               sets the rank min(k, n_g) - 1; the last key pick knows the size of the block of
//               equal keys and how many of it are wanted, and raises `any_cut` when fewer are
//               wanted than there are.  The row passes return at once while no group did
//   emit        one pass over the records: a row at or below its group's threshold takes the
//               next place of the group's k-entry segment (an atomic cursor; arrival order)
//   sort_out    one wave (k <= 64) or one workgroup per group: a bitonic sort of the segment in
//               LDS by (~key high, ~key low, row), then every output - the slot re-read from
//               the batch, the node by a binary search in row_off, the table's own value bits
//               under the node's flag word - and the fill past the count
// No kernel waits on another workgroup.  Every index is clamped (the shared layer's rules; a
// group word by n_groups, a segment place by k, a segment's row by n_rows), so no batch faults.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kacc_derive.hpp"
#include "kacc_internal.hpp"
#include "kacc_rows.hpp"

namespace kacc {
namespace gtop {

constexpr uint32_t kThreads = 512;           // 8 waves
constexpr uint32_t kPer = 8;                 // rows per lane and tile, all in flight together
constexpr uint32_t kTile = kThreads * kPer;  // rows per tile
constexpr uint32_t kDigits = 256;            // counters per group: one digit is 8 bits
constexpr uint32_t kKeyPasses = 8;           // digits per key
constexpr uint32_t kLdsWords = 16384;        // digit_lds: 64 KiB of u32 counters, two workgroups per CU
constexpr uint32_t kLdsGroups = kLdsWords / kDigits;  // 64: more groups count in global memory
constexpr uint32_t kMergeRounds = 4;         // digit_global: merges per row before the plain atomic
constexpr uint32_t kMaxMergeRounds = 8;
constexpr uint32_t kPickThreads = 256;       // pick: four groups per workgroup
constexpr uint32_t kSortThreads = 256;       // sort_out: four groups (k <= 64) or one per workgroup
constexpr uint32_t kWaveK = 64;              // the largest k a wave sorts alone
constexpr uint32_t kErrTop = 1u << 9;        // "top list": an id or a slot past its range, a row range outside the batch
constexpr uint32_t kNone = 0xffffffffu;      // the group word of a row that is not ranked; the fill
static_assert(kDigits == plan::kDigits && kLdsWords == plan::kDigitWords, "the host plans with the kernels' LDS size");
using rows::kCus, rows::knob;  // knob: the tuning knobs of tools/bench_gtop.py
using rows::kDerived, rows::kEnergy, rows::kStored;  // the table of the values

enum Mode { kFirstKey = 0, kKey = 1, kRow = 2 };  // what a digit pass counts
enum Pick { kPickFirst = 0, kPickKey = 1, kPickLastKey = 2, kPickRow = 3 };

struct Args {
  rows::View v;
  // the values' table
  const uint64_t *words;  // energy / stored power words of `zone`: words[slot * v.tab_stride]
  uint32_t zone;
  const uint32_t *group;  // NULL: every row in group 0
  uint32_t n_groups, k, tiles;
  // the grid
  uint32_t copies, stride;  // digit_lds: 2^j copies of the counters, a copy's words apart
  uint32_t merge_rounds;    // digit_global: wave merges before the plain atomic
  uint32_t row_exit;        // the row passes return at once while any_cut is 0
  uint32_t sort_p;          // sort_out: the power of two >= k
  uint32_t node_steps;      // sort_out: ceil(log2(n_nodes))
  // scratch
  uint32_t *bins;      // [n_groups * 256] zero between the passes
  uint64_t *thr;       // [n_groups] the digits of ~key decided so far; after the key passes T_g
  uint32_t *rem;       // [n_groups] the rank that remains among the rows with the prefix
  uint32_t *count;     // [n_groups] n_g
  uint32_t *rthr;      // [n_groups] the row threshold R_g (its digits decided so far in a cut group)
  uint32_t *cut;       // [n_groups] 1: fewer rows of the block of keys equal to T_g are wanted than it has
  uint32_t *cursor;    // [n_groups] emit: the next place of the group's segment
  uint32_t *any_cut;   // [1] some group has a cut block
  uint64_t *row_key;   // [n_rows] ~key
  uint32_t *row_group; // [n_rows]
  uint64_t *seg_key;   // [n_groups * k]
  uint32_t *seg_row;   // [n_groups * k]
  // the outputs
  uint32_t *out_count, *out_row, *out_slot, *out_node;
  uint64_t *out_value;
  uint32_t *err;
};

// One workgroup per tile: ~key and the group word of every row of the batch.
template <int kSrc>
__global__ __launch_bounds__(kThreads) void keys_kernel(const Args a) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  rows::Located<kPer> l;
  rows::locate<kPer>(a.v, a.group, blockIdx.x, kTile, lane, wave, l);
  uint64_t key[kPer];
#pragma unroll
  for (uint32_t u = 0; u < kPer; ++u) {
    rows::check_row(a.v, a.n_groups, l, u);
    uint64_t v = 0;
    if (a.v.cap != 0)  // uniform
      v = rows::value_bits<kSrc>(a.words, a.v.tab_stride, a.v.pd, a.v.Z, a.zone, l.sl[u], l.node[u], l.f[u]);
    key[u] = kSrc == kEnergy ? v : rows::power_key(v);
  }
  if (l.bad) atomicOr(a.err, kErrTop);
#pragma unroll
  for (uint32_t u = 0; u < kPer; ++u) {
    if (!l.in_batch[u]) continue;
    a.row_key[l.r[u]] = ~key[u];  // a NaN (key 0) is all ones: a ranked row, the last of its group
    a.row_group[l.r[u]] = l.ok[u] ? l.g[u] : kNone;
  }
}

struct TileRecords {  // a lane's kPer row records of a tile
  uint64_t key[kPer];  // ~key
  uint32_t row[kPer];
  uint32_t g[kPer];  // the group, clamped
  bool ranked[kPer];
};
// The records of tile `tile`; a row past the batch is clamped to its last row and not ranked.
__device__ __forceinline__ void load_records(const Args &a, uint32_t tile, uint32_t lane, uint32_t wave,
                                             TileRecords &t) {
  const uint64_t row0 = static_cast<uint64_t>(tile) * kTile + wave * (kPer * 64u) + lane;
  const uint32_t last_row = a.v.n_rows - 1;
#pragma unroll
  for (uint32_t u = 0; u < kPer; ++u) {
    const uint64_t rr = row0 + u * 64u;
    const uint32_t r = static_cast<uint32_t>(min(rr, static_cast<uint64_t>(last_row)));
    t.key[u] = a.row_key[r];
    const uint32_t word = a.row_group[r];
    t.row[u] = r;
    t.ranked[u] = rr <= last_row && word != kNone;
    t.g[u] = min(word, a.n_groups - 1u);
  }
}

struct GroupState {  // what a pass knows of a record's group
  uint64_t thr[kPer];
  uint32_t rthr[kPer], cut[kPer];
};
template <int kMode>
__device__ __forceinline__ void load_state(const Args &a, const TileRecords &t, GroupState &s) {
#pragma unroll
  for (uint32_t u = 0; u < kPer; ++u) {
    s.thr[u] = kMode == kFirstKey ? 0 : a.thr[t.g[u]];
    s.rthr[u] = kMode == kRow ? a.rthr[t.g[u]] : 0;
    s.cut[u] = kMode == kRow ? a.cut[t.g[u]] : 0;
  }
}
// Does record u count in this pass, and in which digit?  A key pass: the key carries the digits
// of the prefix above `shift` + 8 (every key does in the first pass).  A row pass: the group has
// a cut block, the key is the group's threshold, and the row carries the row digits decided so far.
template <int kMode>
__device__ __forceinline__ bool counts(const TileRecords &t, const GroupState &s, uint32_t u, uint32_t shift,
                                       uint32_t &digit) {
  if constexpr (kMode == kRow) {
    digit = (t.row[u] >> shift) & (kDigits - 1u);
    const uint64_t diff = static_cast<uint64_t>(t.row[u] ^ s.rthr[u]);
    return t.ranked[u] && s.cut[u] != 0 && t.key[u] == s.thr[u] && (diff >> (shift + 8u)) == 0;
  } else {
    digit = static_cast<uint32_t>(t.key[u] >> shift) & (kDigits - 1u);
    if constexpr (kMode == kFirstKey) return t.ranked[u];
    return t.ranked[u] && ((t.key[u] ^ s.thr[u]) >> (shift + 8u)) == 0;  // shift <= 48 past the first pass
  }
}

// One add per lane that has `todo`, into counter `word`.  First, for `rounds` rounds, the lanes
// that hit the word of the first waiting lane merge into one add of their number.
template <class Add>
__device__ __forceinline__ void merged_add(bool todo, uint32_t word, uint32_t rounds, uint32_t lane, Add add) {
  for (uint32_t round = 0; round < rounds; ++round) {  // uniform
    const uint64_t waiting = __ballot(todo);
    if (waiting == 0) break;  // wave-uniform
    const uint32_t lead = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(__builtin_ctzll(waiting)));
    const uint32_t lead_word = __builtin_amdgcn_readlane(word, lead);
    const bool same = todo && word == lead_word;
    const uint32_t n = static_cast<uint32_t>(__popcll(__ballot(same)));
    if (lane == lead) add(lead_word, n);
    todo = todo && !same;
  }
  if (todo) add(word, 1u);
}

// The counters of every group in LDS, `copies` times; persistent workgroups share the tiles.
template <int kMode>
__global__ __launch_bounds__(kThreads, 4) void digit_lds_kernel(const Args a, const uint32_t shift) {
  __shared__ uint32_t s_bins[kLdsWords];
  if (kMode == kRow && a.row_exit && *a.any_cut == 0) return;  // uniform: no block of equal keys is cut
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  for (uint32_t i = tid; i < a.copies * a.stride; i += kThreads) s_bins[i] = 0;  // <= kLdsWords (host)
  __syncthreads();
  uint32_t *const b = s_bins + (lane & (a.copies - 1u)) * a.stride;
  for (uint32_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {  // workgroup-uniform
    TileRecords t;
    GroupState s;
    load_records(a, tile, lane, wave, t);
    load_state<kMode>(a, t, s);
#pragma unroll
    for (uint32_t u = 0; u < kPer; ++u) {
      uint32_t digit;
      if (counts<kMode>(t, s, u, shift, digit)) atomicAdd(b + t.g[u] * kDigits + digit, 1u);
    }
  }
  __syncthreads();
  for (uint32_t i = tid; i < a.n_groups * kDigits; i += kThreads) {  // consecutive lanes, consecutive words
    uint32_t v = 0;
    for (uint32_t c = 0; c < a.copies; ++c) v += s_bins[c * a.stride + i];
    if (v) atomicAdd(a.bins + i, v);
  }
}

// The counters in global memory.  A fleet of idle processes puts most rows of a group on ONE
// word: the lanes of a wave that hit the word of the first waiting lane merge into one add.
template <int kMode>
__global__ __launch_bounds__(kThreads) void digit_global_kernel(const Args a, const uint32_t shift) {
  if (kMode == kRow && a.row_exit && *a.any_cut == 0) return;  // uniform
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  for (uint32_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {  // workgroup-uniform
    TileRecords t;
    GroupState s;
    load_records(a, tile, lane, wave, t);
    load_state<kMode>(a, t, s);
#pragma unroll
    for (uint32_t u = 0; u < kPer; ++u) {
      uint32_t digit;
      const bool todo = counts<kMode>(t, s, u, shift, digit);
      merged_add(todo, t.g[u] * kDigits + digit /* < 2^24 */, a.merge_rounds, lane,
                 [&](uint32_t w, uint32_t n) { atomicAdd(a.bins + w, n); });
    }
  }
}

// One wave per group: lane l holds counters 4l .. 4l + 3.
__global__ __launch_bounds__(kPickThreads) void pick_kernel(const Args a, const uint32_t shift, const uint32_t what) {
  if (what == kPickRow && a.row_exit && *a.any_cut == 0) return;  // uniform; the counters are zero
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t g = __builtin_amdgcn_readfirstlane(blockIdx.x * (kPickThreads / 64u) + (threadIdx.x >> 6));
  if (g >= a.n_groups) return;  // wave-uniform
  uint4 *const p = reinterpret_cast<uint4 *>(a.bins + static_cast<uint64_t>(g) * kDigits) + lane;
  const uint4 c = *p;
  *p = make_uint4(0u, 0u, 0u, 0u);  // the next pass counts from zero
  const uint32_t mine = c.x + c.y + c.z + c.w;  // a context has fewer than 2^32 rows
  uint32_t incl = mine;
#pragma unroll
  for (uint32_t d = 1; d < 64u; d <<= 1) {
    const uint32_t up = __shfl_up(incl, d);
    if (lane >= d) incl += up;
  }
  uint32_t rem;
  if (what == kPickFirst) {  // uniform: every row of the group was counted, so the counters add to n_g
    const uint32_t n = __shfl(incl, 63);
    rem = n ? min(a.k, n) - 1u : 0u;  // the position of the list's last row
    if (lane == 0) a.count[g] = n;
  } else {
    rem = a.rem[g];
  }
  const uint32_t excl = incl - mine;
  if (excl <= rem && rem < incl) {  // one lane; none in a group without rows or, in a row pass, without a cut
    uint32_t below = excl, d = 0, eq = c.x;
    if (rem >= below + eq) { below += eq; d = 1; eq = c.y; }
    if (d == 1 && rem >= below + eq) { below += eq; d = 2; eq = c.z; }
    if (d == 2 && rem >= below + eq) { below += eq; d = 3; eq = c.w; }
    const uint32_t digit = lane * 4u + d;
    rem -= below;
    a.rem[g] = rem;
    if (what == kPickRow) {
      a.rthr[g] |= digit << shift;  // 0 before the first row pass
    } else {
      a.thr[g] = (what == kPickFirst ? 0ull : a.thr[g]) | static_cast<uint64_t>(digit) << shift;
      if (what == kPickLastKey) {
        // eq rows hold the threshold key, rem + 1 of them are wanted: all of them, or the lowest rows
        const bool cut = rem + 1u < eq;
        a.cut[g] = cut;
        a.rthr[g] = cut ? 0u : kNone;
        if (cut) atomicOr(a.any_cut, 1u);
      }
    }
  }
}

// One pass over the records: the rows of the lists, each into the next place of its group's segment.
__global__ __launch_bounds__(kThreads) void emit_kernel(const Args a) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  for (uint32_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {  // workgroup-uniform
    TileRecords t;
    load_records(a, tile, lane, wave, t);
    uint64_t thr[kPer];
    uint32_t rthr[kPer];
#pragma unroll
    for (uint32_t u = 0; u < kPer; ++u) {
      thr[u] = a.thr[t.g[u]];
      rthr[u] = a.rthr[t.g[u]];
    }
#pragma unroll
    for (uint32_t u = 0; u < kPer; ++u) {
      const bool take = t.ranked[u] && (t.key[u] < thr[u] || (t.key[u] == thr[u] && t.row[u] <= rthr[u]));
      if (take) {
        const uint32_t at = atomicAdd(a.cursor + t.g[u], 1u);
        if (at < a.k) {  // the set is exact: always
          const uint64_t e = static_cast<uint64_t>(t.g[u]) * a.k + at;
          a.seg_key[e] = t.key[u];
          a.seg_row[e] = t.row[u];
        }
      }
    }
  }
}

// (hi, lo, row) ascending: true when a sorts after b
__device__ __forceinline__ bool after(uint2 ak, uint32_t ar, uint2 bk, uint32_t br) {
  return ak.y != bk.y ? ak.y > bk.y : (ak.x != bk.x ? ak.x > bk.x : ar > br);
}

// One wave (kWave: k <= 64, four groups per workgroup) or one workgroup per group: the segment
// sorted by its unique composite, then every non-NULL output of the group.
template <int kSrc, bool kWave>
__global__ __launch_bounds__(kSortThreads) void sort_out_kernel(const Args a) {
  constexpr uint32_t kUnit = kWave ? 64u : kSortThreads;       // threads per group
  constexpr uint32_t kEntries = kWave ? kWaveK : KACC_TOP_MAX;  // LDS entries per group
  __shared__ uint2 s_key[kWave ? kSortThreads : KACC_TOP_MAX];
  __shared__ uint32_t s_row[kWave ? kSortThreads : KACC_TOP_MAX];
  const uint32_t tid = threadIdx.x;
  const uint32_t me = kWave ? (tid & 63u) : tid;
  const uint32_t g = kWave ? __builtin_amdgcn_readfirstlane(blockIdx.x * (kSortThreads / 64u) + (tid >> 6)) : blockIdx.x;
  if (g >= a.n_groups) return;  // wave-uniform (kWave: no workgroup barrier below)
  uint2 *const key = s_key + (kWave ? (tid >> 6) * kWaveK : 0u);
  uint32_t *const row = s_row + (kWave ? (tid >> 6) * kWaveK : 0u);
  auto sync = [&]() {
    if constexpr (kWave) rows::wave_lds_fence(); else __syncthreads();
  };
  const uint32_t k = a.k, P = min(a.sort_p, kEntries);
  const uint32_t cnt = min(k, a.count[g]);
  const uint64_t o = static_cast<uint64_t>(g) * k;
  for (uint32_t i = me; i < P; i += kUnit) {  // a place past the count: the fill, which sorts last
    const uint64_t e = o + (i < cnt ? i : 0u);  // a group's first place is always allocated
    const uint64_t ik = a.seg_key[e];
    const uint32_t r = a.seg_row[e];
    key[i] = i < cnt ? make_uint2(static_cast<uint32_t>(ik), static_cast<uint32_t>(ik >> 32)) : make_uint2(kNone, kNone);
    row[i] = i < cnt ? r : kNone;
  }
  sync();
  for (uint32_t sz = 2; sz <= P; sz <<= 1) {
    for (uint32_t st = sz >> 1; st > 0; st >>= 1) {
      for (uint32_t t = me; t < (P >> 1); t += kUnit) {
        const uint32_t i = 2 * t - (t & (st - 1)), j = i + st;
        const uint2 ki = key[i], kj = key[j];
        const uint32_t ri = row[i], rj = row[j];
        const bool up = (i & sz) == 0;
        if (after(ki, ri, kj, rj) == up) {
          key[i] = kj;
          key[j] = ki;
          row[i] = rj;
          row[j] = ri;
        }
      }
      sync();
    }
  }
  if (me == 0 && a.out_count) a.out_count[g] = cnt;
  const uint32_t last_row = a.v.n_rows - 1;  // not used without a tile
  for (uint32_t j = me; j < k; j += kUnit) {
    const bool in = j < cnt;
    uint32_t r = kNone, sl = kNone, node = kNone;
    uint64_t v = 0;
    if (a.tiles) {  // uniform: there are rows and nodes.  Every load below is clamped, none is skipped
      const uint32_t rc = min(in ? row[j] : 0u, last_row);
      const uint32_t s = a.v.slot[rc] & KACC_SLOT_MASK;
      const uint32_t sc = s < a.v.cap ? s : 0u;  // below the capacity: checked when the row was classified
      uint32_t lo = 0, hi = a.v.n_nodes - 1;
      for (uint32_t step = 0; step < a.node_steps; ++step) rows::node_step(a.v.row_off, rc, lo, hi);  // uniform
      const uint32_t f = a.v.nflags[lo];
      uint64_t bits = 0;
      if (a.v.cap != 0)  // uniform
        bits = rows::value_bits<kSrc>(a.words, a.v.tab_stride, a.v.pd, a.v.Z, a.zone, sc, lo, f);
      r = in ? rc : kNone;
      sl = in ? s : kNone;
      node = in ? lo : kNone;
      v = in ? bits : 0ull;  // the table's own bits: -0.0 stays -0.0, a NaN keeps its payload
    }
    if (a.out_row) a.out_row[o + j] = r;
    if (a.out_slot) a.out_slot[o + j] = sl;
    if (a.out_node) a.out_node[o + j] = node;
    if (a.out_value) a.out_value[o + j] = v;
  }
}

template <int kMode>
void launch_digit(const Args &a, bool lds, uint32_t grid, uint32_t shift, hipStream_t st) {
  if (lds)
    KACC_LAUNCH(digit_lds_kernel<kMode>, dim3(grid), dim3(kThreads), 0, st, a, shift);
  else
    KACC_LAUNCH(digit_global_kernel<kMode>, dim3(grid), dim3(kThreads), 0, st, a, shift);
}

template <int kSrc>
void launch_sort_out(const Args &a, hipStream_t st) {
  if (a.k <= kWaveK)
    KACC_LAUNCH((sort_out_kernel<kSrc, true>), dim3((a.n_groups + kSortThreads / 64u - 1) / (kSortThreads / 64u)),
                dim3(kSortThreads), 0, st, a);
  else
    KACC_LAUNCH((sort_out_kernel<kSrc, false>), dim3(a.n_groups), dim3(kSortThreads), 0, st, a);
}

}  // namespace gtop
}  // namespace kacc

extern "C" {

int kacc_group_top(kacc_ctx *ctx, kacc_table t, uint32_t zone, uint32_t k, const kacc_top_rows *rows,
                   const uint32_t *group, uint32_t n_groups, const uint32_t *node_mask, uint32_t *out_count,
                   uint32_t *out_row, uint32_t *out_slot, uint32_t *out_node, uint64_t *out_value, void *stream) {
  using namespace kacc::gtop;
  const char *fn = "kacc_group_top";
  if (!ctx) return KACC_EINVAL;
  kacc::rows::Table tab;
  Args a{};
  int rc = kacc::rows::resolve_table(ctx, fn, t, zone, &tab);
  if (rc != KACC_OK) return rc;
  if (!rows) return kacc_fail(ctx, KACC_EINVAL, "%s: NULL argument", fn);
  if (k < 1 || k > KACC_TOP_MAX) return kacc_fail(ctx, KACC_EINVAL, "%s: k = %u outside 1 .. %u", fn, k, KACC_TOP_MAX);
  if ((rc = kacc::rows::check_groups(ctx, fn, n_groups)) != KACC_OK) return rc;
  if (static_cast<uint64_t>(n_groups) * k > KACC_GROUP_TOP_MAX_ITEMS)
    return kacc_fail(ctx, KACC_EINVAL, "%s: %u groups x k = %u > %u", fn, n_groups, k, KACC_GROUP_TOP_MAX_ITEMS);
  if (!group && n_groups != 1) return kacc_fail(ctx, KACC_EINVAL, "%s: NULL group with n_groups %u", fn, n_groups);
  if ((rc = kacc::rows::resolve(ctx, fn, tab.kind, rows, node_mask, &a.v)) != KACC_OK) return rc;
  if (!out_count && !out_row && !out_slot && !out_node && !out_value)
    return kacc_fail(ctx, KACC_EINVAL, "%s: no output array", fn);

  kacc::rows::Call call(ctx, fn);
  if ((rc = call.open(stream)) != KACC_OK) return rc;
  hipStream_t st = call.st;

  const uint32_t G = n_groups;
  a.words = tab.words;
  a.zone = zone;
  a.group = group;
  a.n_groups = G;
  a.k = k;
  a.out_count = out_count;
  a.out_row = out_row;
  a.out_slot = out_slot;
  a.out_node = out_node;
  a.out_value = out_value;
  a.err = ctx->d_err;

  // the counters: in LDS while one copy fits (replicated, with an odd stride so that the copies
  // of a counter fall into different banks, while they fit more than once), else in global memory
  const bool lds = G <= knob("KACC_GTOP_LDS_GROUPS", kLdsGroups, kLdsGroups);
  a.merge_rounds = knob("KACC_GTOP_MERGE_ROUNDS", kMergeRounds, kMaxMergeRounds);
  a.row_exit = knob("KACC_GTOP_ROW_EXIT", 1u, 1u);
  a.copies = kacc::plan::digit_copies(G, lds);
  a.stride = G * kDigits | (a.copies > 1 ? 1u : 0u);
  // without a node no row is listed
  a.tiles = a.v.n_nodes ? kacc::rows::tiles_of(a.v.n_rows, kTile) : 0u;
  // persistent grids: two workgroups of 8 waves per CU with the LDS counters, four without
  const uint32_t grid = std::max(1u, std::min(a.tiles, kCus * (lds ? 2u : 4u)));
  a.sort_p = 1;
  while (a.sort_p < k) a.sort_p <<= 1;
  a.node_steps = 0;
  while (a.v.n_nodes > 1 && (1ull << a.node_steps) < a.v.n_nodes) ++a.node_steps;
  // the digits of the row index that can differ: nothing is read back, so the batch's size decides
  uint32_t row_passes = 0;
  while (a.tiles && row_passes < 4 && (static_cast<uint64_t>(a.v.n_rows) - 1) >> (8u * row_passes)) ++row_passes;

  // temporaries, stream ordered: the counters and the groups' state (zeroed), the row records,
  // the segments, the node flags
  const uint64_t n_rows = a.tiles ? a.v.n_rows : 0, ents = static_cast<uint64_t>(G) * k;
  kacc::plan::Layout tmp;
  tmp.add(&a.bins, static_cast<uint64_t>(G) * kDigits, true);
  tmp.add(&a.thr, G, true);
  for (uint32_t **p : {&a.rem, &a.count, &a.rthr, &a.cut, &a.cursor}) tmp.add(p, G, true);
  tmp.add(&a.any_cut, 1, true);
  tmp.add(&a.row_key, n_rows);
  tmp.add(&a.seg_key, ents);
  tmp.add(&a.row_group, n_rows);
  tmp.add(&a.seg_row, ents);
  tmp.add(&a.v.nflags, a.v.n_nodes);
  if ((rc = call.alloc(tmp)) != KACC_OK) return rc;

  const dim3 block(kThreads);
  if (a.v.n_nodes) kacc::rows::launch_node_prep<kThreads>(a.v, a.err, kErrTop, nullptr, st);
  if (a.tiles) {  // else every group is empty: the zeroed state says so
    kacc::rows::dispatch_src(tab.src, [&](auto s) { KACC_LAUNCH(keys_kernel<s()>, dim3(a.tiles), block, 0, st, a); });
    const dim3 pick_grid((G + kPickThreads / 64u - 1) / (kPickThreads / 64u));
    for (uint32_t pass = 0; pass < kKeyPasses; ++pass) {
      const uint32_t shift = 8u * (kKeyPasses - 1u - pass);
      if (pass == 0)
        launch_digit<kFirstKey>(a, lds, grid, shift, st);
      else
        launch_digit<kKey>(a, lds, grid, shift, st);
      const uint32_t what = pass == 0 ? kPickFirst : pass + 1 == kKeyPasses ? kPickLastKey : kPickKey;
      KACC_LAUNCH(pick_kernel, pick_grid, dim3(kPickThreads), 0, st, a, shift, what);
    }
    for (uint32_t pass = 0; pass < row_passes; ++pass) {  // only a cut block of equal keys counts here
      const uint32_t shift = 8u * (row_passes - 1u - pass);
      launch_digit<kRow>(a, lds, grid, shift, st);
      KACC_LAUNCH(pick_kernel, pick_grid, dim3(kPickThreads), 0, st, a, shift, static_cast<uint32_t>(kPickRow));
    }
    KACC_LAUNCH(emit_kernel, dim3(std::max(1u, std::min(a.tiles, kCus * 4u))), block, 0, st, a);
  }
  kacc::rows::dispatch_src(tab.src, [&](auto s) { launch_sort_out<s()>(a, st); });
  return call.finish();
}

}  // extern "C"
