// Exact quantiles of the running workloads by a caller-defined group, on the device
// (DESIGN §4.15).
//
// No reference counterpart: Kepler exports every running workload and leaves `quantile by` to
// the consumer.  Row r of the caller's last interval batch (one workload kind) has one value -
// the element of the table at (its slot, zone) - and is ranked inside group[r] by the top lists'
// u64 sort key.  A query is a (group, phi) pair; its answer is the key at position
// floor(phi * (n - 1)) of the group's n ranked rows, and the key one position up.  Both are found
// by a radix select, eight digits of 8 bits from the top: every step is an integer count or a key
// comparison, so the result is the same bytes for any tiling and any order of the rows.
//
// The rows, their values, their nodes' flag words and the tile prelude are the shared row
// layer's (kacc_rows.hpp); this file adds the keys, the digit counters and the select on top.
//
//   node_prep   the shared layer's: one flag word per node
//   keys        one workgroup per tile of kTile batch rows: every row is classified ONCE into an
//               8-byte key and a 4-byte group word (the id, or kNone for a row that does not
//               contribute or whose power is a NaN; a NaN row adds 1 to nan[g]).  The later
//               passes read these 12 bytes and touch neither slots, nodes nor tables
//   digit       (eight times) a row adds 1 to bins[query][digit of its key] for every query of its
//               group whose prefix - the digits decided so far - its key matches; in the first
//               pass every row matches.  While the n_queries * 256 u32 counters fit a workgroup's
//               LDS they live there (digit_lds: persistent workgroups, LDS adds, replicated per
//               lane subset with an odd stride while they fit more than once, flushed with one
//               global atomic per workgroup and non-zero word); past that digit_global adds into
//               the global counters, after the lanes of a wave that hit the same word as the first
//               waiting lane have merged into one add, for kMergeRounds rounds
//   pick        one wave per query, 4 counters per lane and a wave prefix scan: the digit whose
//               cumulative count passes the rank that remains, the prefix extended by it, the
//               counts below it subtracted.  It zeroes the counters it has read.  The first pick
//               learns n (the sum of the counters) and turns phi into the rank; the last one
//               knows how many rows equal the key it found and so whether the upper position
//               holds the same key
//   succ        for the queries whose upper position holds another key: the smallest key of the
//               group above the lower one, a u64 atomic min that a row issues only when its key
//               is below the word it has just read
//   finish      one thread per query: the keys back to value bits, the weight, the value
// No kernel waits on another workgroup.  Every index is clamped (the shared layer's rules; a
// group word by n_groups), so no batch faults.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kacc_derive.hpp"
#include "kacc_internal.hpp"
#include "kacc_rows.hpp"

namespace kacc {
namespace quant {

constexpr uint32_t kThreads = 512;           // 8 waves
constexpr uint32_t kPer = 8;                 // rows per lane and tile, all in flight together
constexpr uint32_t kTile = kThreads * kPer;  // rows per tile
constexpr uint32_t kDigits = 256;            // counters per query: one digit is 8 bits
constexpr uint32_t kPasses = 8;              // digits per key
constexpr uint32_t kLdsWords = 16384;        // digit_lds: 64 KiB of u32 counters, two workgroups per CU
constexpr uint32_t kLdsQueries = kLdsWords / kDigits;  // 64: more queries count in global memory
constexpr uint32_t kMergeRounds = 4;         // digit_global: merges per row and query before the plain atomic
constexpr uint32_t kMaxMergeRounds = 8;
constexpr uint32_t kPickThreads = 256;       // pick: four queries per workgroup
constexpr uint32_t kErrQuant = 1u << 15;     // a group id or a slot past its range, a row range outside the batch
constexpr uint32_t kNone = 0xffffffffu;      // the group word of a row that is not ranked
constexpr uint64_t kEmptyNan = 0x7ff8000000000001ull;    // out_value of a group without ranked rows
constexpr uint64_t kInvalidNan = 0xfff8000000000000ull;  // out_value of Inf * 0 and Inf - Inf (header)
static_assert(kDigits == plan::kDigits && kLdsWords == plan::kDigitWords, "the host plans with the kernels' LDS size");
using rows::kCus, rows::knob;  // knob: the tuning knobs of tools/bench_quant.py
using rows::kDerived, rows::kEnergy, rows::kStored;  // the table of the values

struct Args {
  rows::View v;
  // the values' table
  const uint64_t *words;  // energy / stored power words of `zone`: words[slot * v.tab_stride]
  uint32_t zone, power;
  const uint32_t *group;  // NULL: every row in group 0
  uint32_t n_groups, n_phi, n_queries, tiles;  // query g * n_phi + j is (group g, phi[j])
  double phi[KACC_QUANT_MAX_PHI];
  // the grid
  uint32_t copies, stride;  // digit_lds: 2^k copies of the counters, a copy's words apart
  uint32_t merge_rounds;    // digit_global: wave merges before the plain atomic
  // scratch
  uint32_t *bins;      // [n_queries * 256] zero between the passes
  uint64_t *prefix;    // [n_queries] the digits decided so far; after the last pass the lower key
  uint64_t *succ;      // [n_queries] the upper key
  uint32_t *rem;       // [n_queries] the rank that remains among the keys with the prefix
  uint32_t *lower;     // [n_queries] floor(phi * (n - 1))
  uint32_t *count;     // [n_queries] n of the query's group
  uint32_t *nan;       // [n_groups]
  uint64_t *row_key;   // [n_rows]
  uint32_t *row_group; // [n_rows]
  // the outputs
  uint64_t *out_count, *out_nan, *out_lo, *out_hi;
  double *out_weight, *out_value;
  uint32_t *err;
};

// One workgroup per tile: the key and the group word of every row of the batch.
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
  if (l.bad) atomicOr(a.err, kErrQuant);
#pragma unroll
  for (uint32_t u = 0; u < kPer; ++u) {
    if (!l.in_batch[u]) continue;
    const bool nan = kSrc != kEnergy && key[u] == 0;  // only a NaN has key 0
    if (l.ok[u] && nan) atomicAdd(a.nan + l.g[u], 1u);  // rare: the sign of a broken input
    a.row_key[l.r[u]] = key[u];
    a.row_group[l.r[u]] = l.ok[u] && !nan ? l.g[u] : kNone;
  }
}

struct TileRecords {  // a lane's kPer row records of a tile
  uint64_t key[kPer];
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
    t.ranked[u] = rr <= last_row && word != kNone;
    t.g[u] = min(word, a.n_groups - 1u);
  }
}
// Does the key carry the digits of the prefix above `shift` + 8 ?  (Every key does in the first pass.)
template <bool kFirst>
__device__ __forceinline__ bool matches(uint64_t key, uint64_t prefix, uint32_t shift) {
  if constexpr (kFirst) return true;
  return ((key ^ prefix) >> (shift + 8u)) == 0;  // shift <= 48 past the first pass
}

// One add per lane that has `todo`, into counter `word`.  First, for `rounds` rounds, the lanes
// that hit the word of the first waiting lane merge into one add of their number (measured: it
// pays for the global counters only).
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

// The counters of every query in LDS, `copies` times; persistent workgroups share the tiles.
template <bool kFirst>
__global__ __launch_bounds__(kThreads, 4) void digit_lds_kernel(const Args a, const uint32_t shift) {
  __shared__ uint32_t s_bins[kLdsWords];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  for (uint32_t i = tid; i < a.copies * a.stride; i += kThreads) s_bins[i] = 0;  // <= kLdsWords (host)
  __syncthreads();
  uint32_t *const b = s_bins + (lane & (a.copies - 1u)) * a.stride;
  for (uint32_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {  // workgroup-uniform
    TileRecords t;
    load_records(a, tile, lane, wave, t);
    for (uint32_t j = 0; j < a.n_phi; ++j) {  // uniform
      uint64_t prefix[kPer];
#pragma unroll
      for (uint32_t u = 0; u < kPer; ++u) prefix[u] = kFirst ? 0 : a.prefix[t.g[u] * a.n_phi + j];
#pragma unroll
      for (uint32_t u = 0; u < kPer; ++u) {
        const uint32_t digit = static_cast<uint32_t>(t.key[u] >> shift) & (kDigits - 1u);
        if (t.ranked[u] && matches<kFirst>(t.key[u], prefix[u], shift))
          atomicAdd(b + (t.g[u] * a.n_phi + j) * kDigits + digit, 1u);
      }
    }
  }
  __syncthreads();
  for (uint32_t i = tid; i < a.n_queries * kDigits; i += kThreads) {  // consecutive lanes, consecutive words
    uint32_t v = 0;
    for (uint32_t c = 0; c < a.copies; ++c) v += s_bins[c * a.stride + i];
    if (v) atomicAdd(a.bins + i, v);
  }
}

// The counters in global memory.  A fleet of idle processes puts most rows of a group on ONE
// word: the lanes of a wave that hit the word of the first waiting lane merge into one add.
template <bool kFirst>
__global__ __launch_bounds__(kThreads) void digit_global_kernel(const Args a, const uint32_t shift) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  for (uint32_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {  // workgroup-uniform
    TileRecords t;
    load_records(a, tile, lane, wave, t);
    for (uint32_t j = 0; j < a.n_phi; ++j) {  // uniform
      uint64_t prefix[kPer];
#pragma unroll
      for (uint32_t u = 0; u < kPer; ++u) prefix[u] = kFirst ? 0 : a.prefix[t.g[u] * a.n_phi + j];
#pragma unroll
      for (uint32_t u = 0; u < kPer; ++u) {
        const uint32_t digit = static_cast<uint32_t>(t.key[u] >> shift) & (kDigits - 1u);
        const uint32_t word = (t.g[u] * a.n_phi + j) * kDigits + digit;  // < 2^24
        merged_add(t.ranked[u] && matches<kFirst>(t.key[u], prefix[u], shift), word, a.merge_rounds, lane,
                   [&](uint32_t w, uint32_t n) { atomicAdd(a.bins + w, n); });
      }
    }
  }
}

// Prometheus' rank of phi among n > 0 rows: one IEEE multiply.
__device__ __forceinline__ double rank_of(double phi, uint32_t n) { return phi * static_cast<double>(n - 1u); }

// One wave per query: lane l holds counters 4l .. 4l + 3.
__global__ __launch_bounds__(kPickThreads) void pick_kernel(const Args a, const uint32_t shift, const uint32_t first) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t q = __builtin_amdgcn_readfirstlane(blockIdx.x * (kPickThreads / 64u) + (threadIdx.x >> 6));
  if (q >= a.n_queries) return;  // wave-uniform
  uint4 *const p = reinterpret_cast<uint4 *>(a.bins + static_cast<uint64_t>(q) * kDigits) + lane;
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
  if (first) {  // uniform: every row of the group was counted, so the counters add to n
    const uint32_t n = __shfl(incl, 63);
    const uint32_t j = q % a.n_phi;
    rem = n ? static_cast<uint32_t>(floor(rank_of(a.phi[j], n))) : 0u;
    if (lane == 0) {
      a.count[q] = n;
      a.lower[q] = rem;
    }
  } else {
    rem = a.rem[q];
  }
  const uint32_t excl = incl - mine;
  if (excl <= rem && rem < incl) {  // one lane; none in a group without ranked rows
    uint32_t below = excl, d = 0, eq = c.x;
    if (rem >= below + eq) { below += eq; d = 1; eq = c.y; }
    if (d == 1 && rem >= below + eq) { below += eq; d = 2; eq = c.z; }
    if (d == 2 && rem >= below + eq) { below += eq; d = 3; eq = c.w; }
    const uint64_t prefix = (first ? 0ull : a.prefix[q]) | static_cast<uint64_t>(lane * 4u + d) << shift;
    rem -= below;
    a.prefix[q] = prefix;
    a.rem[q] = rem;
    if (shift == 0) {
      // eq rows hold the lower key and the lower position is the rem-th of them: the upper
      // position holds the same key unless it does not exist or the lower one is the last of them
      const bool other = a.lower[q] + 1u < a.count[q] && rem + 1u == eq;
      a.succ[q] = other ? ~0ull : prefix;  // ~0: succ_kernel finds the smallest key above
    }
  }
}

// The upper key of the queries that wait for one (succ == ~0 or what the rows so far made of it).
__global__ __launch_bounds__(kThreads) void succ_kernel(const Args a) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  for (uint32_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {  // workgroup-uniform
    TileRecords t;
    load_records(a, tile, lane, wave, t);
    for (uint32_t j = 0; j < a.n_phi; ++j) {  // uniform
      uint64_t lo[kPer], cur[kPer];
#pragma unroll
      for (uint32_t u = 0; u < kPer; ++u) {
        lo[u] = a.prefix[t.g[u] * a.n_phi + j];
        cur[u] = a.succ[t.g[u] * a.n_phi + j];
      }
#pragma unroll
      for (uint32_t u = 0; u < kPer; ++u)
        if (t.ranked[u] && t.key[u] > lo[u] && t.key[u] < cur[u])
          atomicMin(reinterpret_cast<unsigned long long *>(a.succ + t.g[u] * a.n_phi + j),
                    static_cast<unsigned long long>(t.key[u]));
    }
  }
}

// One thread per query: every non-NULL output.
__global__ __launch_bounds__(kThreads) void finish_kernel(const Args a) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= a.n_queries) return;
  const uint32_t g = i / a.n_phi, j = i - g * a.n_phi;
  const uint32_t n = a.count[i];
  if (j == 0) {
    if (a.out_count) a.out_count[g] = n;
    if (a.out_nan) a.out_nan[g] = a.nan[g];
  }
  uint64_t lo = 0, hi = 0, value = kEmptyNan;
  double weight = 0.0;
  if (n) {
    double phi = a.phi[0];
#pragma unroll
    for (uint32_t k = 1; k < KACC_QUANT_MAX_PHI; ++k) phi = k == j ? a.phi[k] : phi;  // no indexed argument
    const double rank = rank_of(phi, n);
    weight = rank - floor(rank);
    lo = a.prefix[i];
    hi = a.succ[i];
    double dlo, dhi;
    if (a.power) {  // uniform
      lo = rows::power_key_bits(lo);
      hi = rows::power_key_bits(hi);
      dlo = __longlong_as_double(static_cast<long long>(lo));
      dhi = __longlong_as_double(static_cast<long long>(hi));
    } else {
      dlo = static_cast<double>(lo);  // correctly rounded
      dhi = static_cast<double>(hi);
    }
    const double v = dlo * (1.0 - weight) + dhi * weight;  // no FMA: -ffp-contract=off
    // neither operand is a NaN, so a NaN here is an invalid operation's (Inf * 0, Inf - Inf):
    // IEEE leaves its bits open, the header fixes them
    value = v != v ? kInvalidNan : static_cast<uint64_t>(__double_as_longlong(v));
  }
  if (a.out_lo) a.out_lo[i] = lo;
  if (a.out_hi) a.out_hi[i] = hi;
  if (a.out_weight) a.out_weight[i] = weight;
  if (a.out_value) a.out_value[i] = __longlong_as_double(static_cast<long long>(value));
}

}  // namespace quant
}  // namespace kacc

extern "C" {

int kacc_group_quantiles(kacc_ctx *ctx, kacc_table t, uint32_t zone, const kacc_top_rows *rows, const uint32_t *group,
                         uint32_t n_groups, const double *phi, uint32_t n_phi, const uint32_t *node_mask,
                         uint64_t *out_count, uint64_t *out_nan, uint64_t *out_lo, uint64_t *out_hi,
                         double *out_weight, double *out_value, void *stream) {
  using namespace kacc::quant;
  const char *fn = "kacc_group_quantiles";
  if (!ctx) return KACC_EINVAL;
  kacc::rows::Table tab;
  Args a{};
  int rc = kacc::rows::resolve_table(ctx, fn, t, zone, &tab);
  if (rc != KACC_OK) return rc;
  if (!rows || !phi) return kacc_fail(ctx, KACC_EINVAL, "%s: NULL argument", fn);
  if (n_phi < 1 || n_phi > KACC_QUANT_MAX_PHI)
    return kacc_fail(ctx, KACC_EINVAL, "%s: n_phi %u outside 1 .. %u", fn, n_phi, KACC_QUANT_MAX_PHI);
  if ((rc = kacc::rows::check_groups(ctx, fn, n_groups)) != KACC_OK) return rc;
  if (static_cast<uint64_t>(n_groups) * n_phi > KACC_QUANT_MAX_QUERIES)
    return kacc_fail(ctx, KACC_EINVAL, "%s: %u groups x %u quantiles > %u", fn, n_groups, n_phi, KACC_QUANT_MAX_QUERIES);
  if (!group && n_groups != 1) return kacc_fail(ctx, KACC_EINVAL, "%s: NULL group with n_groups %u", fn, n_groups);
  if ((rc = kacc::rows::resolve(ctx, fn, tab.kind, rows, node_mask, &a.v)) != KACC_OK) return rc;
  for (uint32_t j = 0; j < n_phi; ++j) {  // the host array is read here, before the call returns
    if (!(phi[j] >= 0.0 && phi[j] <= 1.0)) return kacc_fail(ctx, KACC_EINVAL, "%s: phi[%u] is not in [0, 1]", fn, j);
    a.phi[j] = phi[j];
  }
  if (!out_count && !out_nan && !out_lo && !out_hi && !out_weight && !out_value)
    return kacc_fail(ctx, KACC_EINVAL, "%s: no output array", fn);

  kacc::rows::Call call(ctx, fn);
  if ((rc = call.open(stream)) != KACC_OK) return rc;
  hipStream_t st = call.st;

  const uint32_t Q = n_groups * n_phi;
  a.words = tab.words;
  a.zone = zone;
  a.power = tab.power;
  a.group = group;
  a.n_groups = n_groups;
  a.n_phi = n_phi;
  a.n_queries = Q;
  a.out_count = out_count;
  a.out_nan = out_nan;
  a.out_lo = out_lo;
  a.out_hi = out_hi;
  a.out_weight = out_weight;
  a.out_value = out_value;
  a.err = ctx->d_err;

  // the counters: in LDS while one copy fits (replicated, with an odd stride so that the copies
  // of a counter fall into different banks, while they fit more than once), else in global memory
  const bool lds = Q <= knob("KACC_QUANT_LDS_QUERIES", kLdsQueries, kLdsQueries);
  a.merge_rounds = knob("KACC_QUANT_MERGE_ROUNDS", kMergeRounds, kMaxMergeRounds);
  a.copies = kacc::plan::digit_copies(Q, lds);
  a.stride = Q * kDigits | (a.copies > 1 ? 1u : 0u);
  // without a node no row is listed
  a.tiles = a.v.n_nodes ? kacc::rows::tiles_of(a.v.n_rows, kTile) : 0u;
  // persistent grids: two workgroups of 8 waves per CU with the LDS counters, four without
  const uint32_t grid = std::max(1u, std::min(a.tiles, kCus * (lds ? 2u : 4u)));

  // temporaries, stream ordered: the counters and the queries' state (zeroed), the row records, the node flags
  const uint64_t n_rows = a.tiles ? a.v.n_rows : 0;
  kacc::plan::Layout tmp;
  tmp.add(&a.bins, static_cast<uint64_t>(Q) * kDigits, true);
  for (uint64_t **p : {&a.prefix, &a.succ}) tmp.add(p, Q, true);
  for (uint32_t **p : {&a.rem, &a.lower, &a.count}) tmp.add(p, Q, true);
  tmp.add(&a.nan, n_groups, true);
  tmp.add(&a.row_key, n_rows);
  tmp.add(&a.row_group, n_rows);
  tmp.add(&a.v.nflags, a.v.n_nodes);
  if ((rc = call.alloc(tmp)) != KACC_OK) return rc;

  const dim3 block(kThreads);
  if (a.v.n_nodes) kacc::rows::launch_node_prep<kThreads>(a.v, a.err, kErrQuant, nullptr, st);
  if (a.tiles) {  // else every group is empty: the zeroed state says so
    kacc::rows::dispatch_src(tab.src, [&](auto s) { KACC_LAUNCH(keys_kernel<s()>, dim3(a.tiles), block, 0, st, a); });
    const dim3 pick_grid((Q + kPickThreads / 64u - 1) / (kPickThreads / 64u));
    for (uint32_t pass = 0; pass < kPasses; ++pass) {
      const uint32_t shift = 8u * (kPasses - 1u - pass);
      if (lds && pass == 0)
        KACC_LAUNCH(digit_lds_kernel<true>, dim3(grid), block, 0, st, a, shift);
      else if (lds)
        KACC_LAUNCH(digit_lds_kernel<false>, dim3(grid), block, 0, st, a, shift);
      else if (pass == 0)
        KACC_LAUNCH(digit_global_kernel<true>, dim3(grid), block, 0, st, a, shift);
      else
        KACC_LAUNCH(digit_global_kernel<false>, dim3(grid), block, 0, st, a, shift);
      KACC_LAUNCH(pick_kernel, pick_grid, dim3(kPickThreads), 0, st, a, shift, pass == 0 ? 1u : 0u);
    }
    KACC_LAUNCH(succ_kernel, dim3(grid), block, 0, st, a);
  }
  KACC_LAUNCH(finish_kernel, dim3((Q + kThreads - 1) / kThreads), block, 0, st, a);
  return call.finish();
}

}  // extern "C"
