// Running workloads summed by a caller-defined group, on the device.
//
// No reference counterpart: Kepler exports every running workload and leaves `sum by (label)` to
// PromQL.  Row r of the caller's last interval batch (one workload kind) adds its Z-word energy
// record and its Z powers, as fixed-point integers of 2^-12 µW, into the sums of group[r].
// Every sum is an integer mod 2^64, so the order of the additions is free and the result is the
// same bits for any tiling, any shard split and any number of GPUs.
//
// The rows, their nodes' flag words, the tile prelude and the pass queue are the shared row
// layer's (kacc_rows.hpp); this file adds the group bins on top.
//
//   node_prep   the shared layer's: one flag word per node
//   bin         the groups' bins (count | dropped, Z energies, Z powers) fit in LDS: persistent
//               workgroups, each walks every splits-th tile of kTile batch rows (located by the
//               shared prelude), gathers every contributing row's record and adds it with
//               64-bit LDS adds.  A group count small enough is replicated per lane subset, so
//               the lanes of a wave do not queue on one bin
//   rows, pass  more groups than LDS holds: `rows` classifies every row ONCE (one workgroup per
//               tile) into a row word - the group id and the node's guard bits, or "no group" -
//               and the row's node.  `pass` is a grid of passes x splits persistent workgroups;
//               a pass owns a range of `bins` groups.  Every workgroup reads the tile's 4-byte row
//               words; only the workgroup whose pass owns the row's group gathers its record
//   flush       (the end of bin and pass) a workgroup adds its non-zero bins into the zeroed
//               accumulator with u64 atomics, consecutive lanes on consecutive words: one atomic
//               per workgroup and bin word, never one per row
//   finish      one thread per accumulator word: the outputs, and out_power from out_power_fx
// Every index is clamped (the shared layer's rules; group ids by the pass's range), so no batch
// faults.
#include <hip/hip_runtime.h>

#include "kacc_derive.hpp"
#include "kacc_internal.hpp"
#include "kacc_rows.hpp"

namespace kacc {
namespace grp {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kPer = 8;                      // rows per lane and tile
constexpr uint32_t kChunk = 4;                    // rows whose records a lane has in flight together
constexpr uint32_t kTile = kThreads * kPer;       // rows per tile
constexpr uint32_t kSmallWords = 4096;            // u64 of LDS bins: 32 KiB, three workgroups per CU
constexpr uint32_t kBigWords = 9984;              // 78 KiB, two workgroups per CU: 1,109 groups at Z = 4
constexpr uint32_t kPassWords = 9728;             // a pass's bins: 76 KiB, 1,080 groups at Z = 4
static_assert(kSmallWords == plan::kGroupLds.small_words && kBigWords == plan::kGroupLds.big_words &&
                  kPassWords == plan::kGroupLds.pass_words, "the host plans with the kernels' LDS sizes");
constexpr uint32_t kPassTile = kThreads * rows::kPassPer;  // the queues: 2 KiB per workgroup
constexpr uint32_t kErrGroup = 1u << 13;          // a group id or a slot past its range, a row range
                                                  // outside the batch
// the row word of the `rows` pass: the group id, the node's guard bits above it
constexpr uint32_t kWordGroup = 0xffffu, kWordGuardShift = 16;
static_assert(KACC_GROUP_MAX <= kWordGroup + 1u && KACC_MAX_ZONES <= 8u, "a row word holds the id and the guard bits");
using rows::derived_bits, rows::kQueue, rows::lds_add;
using u64x2 = __attribute__((ext_vector_type(2))) unsigned long long;

struct Args {
  rows::View v;
  const uint32_t *group;
  uint32_t n_groups, tiles;
  // the grid
  uint32_t splits;                // workgroups that share the tiles
  uint32_t copies, copy_stride;   // bin: 2^k copies of the bins, copy_stride u64 apart
  uint32_t bins, passes;          // pass: groups per pass; workgroup b takes pass b % passes, split b / passes
  // scratch
  uint64_t *acc;     // [n_groups] count | dropped << 32, [n_groups * Z] energy, [n_groups * Z] power_fx
  uint32_t *row_word, *row_node;  // [n_rows] (pass only)
  // the outputs
  uint32_t *out_count, *out_dropped;
  uint64_t *out_e, *out_fx;
  double *out_p;
  uint32_t *err;
};

// fx(p) of the header for the f64 with these bits; a dropped value counts in `dropped`.
__device__ __forceinline__ uint64_t fx_or_drop(uint64_t bits, uint32_t &dropped) {
  bool keep;
  const uint64_t fx = rows::power_fx(bits, keep);
  dropped += !keep;
  return fx;
}

// The tile's rows, located and checked (the shared prelude): t.ok is "the row contributes".
__device__ __forceinline__ void locate_tile(const Args &a, uint32_t tile, uint32_t lane, uint32_t wave,
                                            rows::Located<kPer> &t) {
  rows::locate<kPer>(a.v, a.group, tile, kTile, lane, wave, t);
#pragma unroll
  for (uint32_t u = 0; u < kPer; ++u) rows::check_row(a.v, a.n_groups, t, u);
}

// Adds one row's record (slot sl below the capacity, its node, the node's guard bits f) into bin
// `bin` of b_cd / b_e / b_p.  kZ: the zone count when it is 4 (16-byte loads), else 0: any Z.
template <uint32_t kZ>
__device__ __forceinline__ void add_one(const Args &a, uint32_t sl, uint32_t node, uint32_t f, uint32_t bin,
                                        uint64_t *b_cd, uint64_t *b_e, uint64_t *b_p) {
  const uint32_t Z = kZ ? kZ : a.v.Z;
  const uint64_t *se = a.v.tab_e + static_cast<uint64_t>(sl) * a.v.tab_stride;
  const uint64_t *sp = a.v.derived ? reinterpret_cast<const uint64_t *>(a.v.pd.active_power) + static_cast<uint64_t>(node) * Z
                                 : a.v.tab_p + static_cast<uint64_t>(sl) * a.v.tab_stride;
  const double ratio = a.v.derived ? a.v.pd.ratio[sl] : 0.0;
  uint32_t dropped = 0;
  if constexpr (kZ == 4) {
    const u64x2 e0 = reinterpret_cast<const u64x2 *>(se)[0], e1 = reinterpret_cast<const u64x2 *>(se)[1];
    const u64x2 p0 = reinterpret_cast<const u64x2 *>(sp)[0], p1 = reinterpret_cast<const u64x2 *>(sp)[1];
    const uint64_t ew[4] = {e0.x, e0.y, e1.x, e1.y}, pw[4] = {p0.x, p0.y, p1.x, p1.y};
#pragma unroll
    for (uint32_t z = 0; z < 4; ++z) {
      const uint64_t bits =
          a.v.derived ? derived_bits(f, z, ratio, __longlong_as_double(static_cast<long long>(pw[z]))) : pw[z];
      lds_add(&b_e[bin * 4u + z], ew[z]);
      lds_add(&b_p[bin * 4u + z], fx_or_drop(bits, dropped));
    }
  } else {
    for (uint32_t z = 0; z < Z; ++z) {
      const uint64_t pw = sp[z];
      const uint64_t bits = a.v.derived ? derived_bits(f, z, ratio, __longlong_as_double(static_cast<long long>(pw))) : pw;
      lds_add(&b_e[bin * Z + z], se[z]);
      lds_add(&b_p[bin * Z + z], fx_or_drop(bits, dropped));
    }
  }
  lds_add(&b_cd[bin], 1ull | static_cast<uint64_t>(dropped) << 32);
}

// Adds the records of the rows that are `mine` into the bins b_cd / b_e / b_p of nloc groups.
// kZ: the zone count when it is 4 (a lane keeps kChunk rows' records in registers, 16-byte
// loads; every row's record is loaded, the slots are clamped, so no load sits behind a
// data-dependent branch), else 0: any Z, word by word.
template <uint32_t kZ>
__device__ __forceinline__ void add_rows(const Args &a, const bool (&mine)[kPer], const uint32_t (&sl)[kPer],
                                         const uint32_t (&node)[kPer], const uint32_t (&f)[kPer],
                                         const uint32_t (&bin)[kPer], uint64_t *b_cd, uint64_t *b_e, uint64_t *b_p) {
  if constexpr (kZ == 4) {
#pragma unroll
    for (uint32_t c = 0; c < kPer; c += kChunk) {
      u64x2 e[kChunk][2], p[kChunk][2];
      double ratio[kChunk];
#pragma unroll
      for (uint32_t j = 0; j < kChunk; ++j) {
        const uint32_t u = c + j;
        e[j][0] = e[j][1] = p[j][0] = p[j][1] = u64x2{0ull, 0ull};
        ratio[j] = 0.0;
        if (a.v.cap != 0) {  // uniform
          const u64x2 *se = reinterpret_cast<const u64x2 *>(a.v.tab_e + static_cast<uint64_t>(sl[u]) * a.v.tab_stride);
          e[j][0] = se[0];
          e[j][1] = se[1];
          const u64x2 *sp;
          if (a.v.derived) {  // uniform
            ratio[j] = a.v.pd.ratio[sl[u]];
            sp = reinterpret_cast<const u64x2 *>(a.v.pd.active_power + static_cast<uint64_t>(node[u]) * 4u);
          } else {
            sp = reinterpret_cast<const u64x2 *>(a.v.tab_p + static_cast<uint64_t>(sl[u]) * a.v.tab_stride);
          }
          p[j][0] = sp[0];
          p[j][1] = sp[1];
        }
      }
#pragma unroll
      for (uint32_t j = 0; j < kChunk; ++j) {
        const uint32_t u = c + j;
        if (!mine[u]) continue;
        const uint64_t ew[4] = {e[j][0].x, e[j][0].y, e[j][1].x, e[j][1].y};
        const uint64_t pw[4] = {p[j][0].x, p[j][0].y, p[j][1].x, p[j][1].y};
        uint32_t dropped = 0;
#pragma unroll
        for (uint32_t z = 0; z < 4; ++z) {
          const uint64_t bits =
              a.v.derived ? derived_bits(f[u], z, ratio[j], __longlong_as_double(static_cast<long long>(pw[z]))) : pw[z];
          lds_add(&b_e[bin[u] * 4u + z], ew[z]);
          lds_add(&b_p[bin[u] * 4u + z], fx_or_drop(bits, dropped));
        }
        lds_add(&b_cd[bin[u]], 1ull | static_cast<uint64_t>(dropped) << 32);
      }
    }
  } else {
#pragma unroll
    for (uint32_t u = 0; u < kPer; ++u)
      if (mine[u]) add_one<0>(a, sl[u], node[u], f[u], bin[u], b_cd, b_e, b_p);
  }
}

// The flush: word i of the workgroup's bins of groups [g0, g0 + nloc) (the copies summed) into
// the accumulator's planes, consecutive lanes on consecutive words.
__device__ __forceinline__ void flush_bins(const Args &a, const uint64_t *s_bin, uint32_t copies, uint32_t g0,
                                           uint32_t nloc, uint32_t tid) {
  const uint32_t Z = a.v.Z, n_e = nloc * Z;
  for (uint32_t i = tid; i < nloc + 2u * n_e; i += kThreads) {
    uint64_t v = 0;
    for (uint32_t c = 0; c < copies; ++c) v += s_bin[c * a.copy_stride + i];
    if (v == 0) continue;
    uint64_t *dst;
    if (i < nloc)
      dst = a.acc + g0 + i;
    else if (i < nloc + n_e)
      dst = a.acc + a.n_groups + static_cast<uint64_t>(g0) * Z + (i - nloc);
    else
      dst = a.acc + a.n_groups + static_cast<uint64_t>(a.n_groups) * Z + static_cast<uint64_t>(g0) * Z + (i - nloc - n_e);
    atomicAdd(reinterpret_cast<unsigned long long *>(dst), static_cast<unsigned long long>(v));
  }
}

// Every group's bins in LDS, `copies` times.
template <uint32_t kZ, uint32_t kLds>
__global__ __launch_bounds__(kThreads, kLds == kSmallWords ? 3 : 2) void bin_kernel(const Args a) {
  __shared__ uint64_t s_bin[kLds];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t Z = kZ ? kZ : a.v.Z, G = a.n_groups;
  for (uint32_t i = tid; i < a.copies * a.copy_stride; i += kThreads) s_bin[i] = 0;  // <= kLds (host)
  __syncthreads();
  uint64_t *const b_cd = s_bin + (lane & (a.copies - 1u)) * a.copy_stride;
  uint64_t *const b_e = b_cd + G, *const b_p = b_e + G * Z;
  bool bad = false;
  for (uint32_t tile = blockIdx.x; tile < a.tiles; tile += a.splits) {  // workgroup-uniform
    rows::Located<kPer> t;
    locate_tile(a, tile, lane, wave, t);
    bad = t.bad || bad;
    add_rows<kZ>(a, t.ok, t.sl, t.node, t.f, t.g, b_cd, b_e, b_p);
  }
  if (bad) atomicOr(a.err, kErrGroup);
  __syncthreads();
  flush_bins(a, s_bin, a.copies, 0u, G, tid);
}

// One workgroup per tile: the row word (group id | guard bits << 16, or KACC_GROUP_NONE for a
// row that does not contribute) and the node of every row of the batch.
__global__ __launch_bounds__(kThreads) void rows_kernel(const Args a) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  rows::Located<kPer> t;
  locate_tile(a, blockIdx.x, lane, wave, t);
  if (t.bad) atomicOr(a.err, kErrGroup);
#pragma unroll
  for (uint32_t u = 0; u < kPer; ++u) {
    if (!t.in_batch[u]) continue;
    a.row_word[t.r[u]] = t.ok[u] ? t.g[u] | (t.f[u] & ((1u << KACC_MAX_ZONES) - 1u)) << kWordGuardShift : KACC_GROUP_NONE;
    a.row_node[t.r[u]] = t.node[u];
  }
}

// A pass's range of groups in LDS; the rows by their row words.  About one row word in `passes`
// is the pass's, so a wave first queues its rows (ballot and popcount, in LDS) and gathers 64
// queued rows at a time, one per lane: the records' loads of 64 rows are in flight together.
template <uint32_t kZ>
__global__ __launch_bounds__(kThreads, 2) void pass_kernel(const Args a) {
  __shared__ uint64_t s_bin[kPassWords];
  __shared__ uint32_t s_q[kThreads / 64][kQueue];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t Z = kZ ? kZ : a.v.Z;
  const uint32_t pass = blockIdx.x % a.passes, split = blockIdx.x / a.passes;
  const uint32_t g0 = pass * a.bins;  // < n_groups
  const uint32_t nloc = min(a.bins, a.n_groups - g0);
  for (uint32_t i = tid; i < nloc * (1u + 2u * Z); i += kThreads) s_bin[i] = 0;  // <= kPassWords (host)
  __syncthreads();
  uint64_t *const b_cd = s_bin, *const b_e = b_cd + nloc, *const b_p = b_e + nloc * Z;
  uint32_t *const q = s_q[wave];
  const uint32_t last_row = a.v.n_rows - 1;

  // the queued rows q[0 .. n) of this wave, n <= 64, one per lane
  auto drain = [&](uint32_t n) {
    if (lane >= n) return;
    const uint32_t r = min(q[lane], last_row);
    const uint32_t word = a.row_word[r];
    const uint32_t bin = min((word & kWordGroup) - g0, nloc - 1u);  // the pass's: checked when it was queued
    const uint32_t s = a.v.slot[r] & KACC_SLOT_MASK;
    const uint32_t sl = s < a.v.cap ? s : 0u;  // below the capacity when the row word was written
    const uint32_t node = min(a.row_node[r], a.v.n_nodes - 1u);
    add_one<kZ>(a, sl, node, word >> kWordGuardShift, bin, b_cd, b_e, b_p);
  };

  rows::pass_queue<kThreads>(
      a.row_word, a.v.n_rows, split, a.splits, lane, wave, q,
      [&](uint32_t word) { return word != KACC_GROUP_NONE && (word & kWordGroup) - g0 < nloc; }, drain);
  __syncthreads();
  flush_bins(a, s_bin, 1u, g0, nloc, tid);
}

// Every non-NULL output of every group out of the accumulator; out_power is the i64 sum,
// correctly rounded to f64, times 2^-12 (exact).
__global__ __launch_bounds__(kThreads) void finish_kernel(const Args a) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
  const uint64_t G = a.n_groups, GZ = G * a.v.Z;
  if (i < G) {
    const uint64_t cd = a.acc[i];
    if (a.out_count) a.out_count[i] = static_cast<uint32_t>(cd);
    if (a.out_dropped) a.out_dropped[i] = static_cast<uint32_t>(cd >> 32);
  }
  if (i < GZ) {
    const uint64_t fx = a.acc[G + GZ + i];
    if (a.out_e) a.out_e[i] = a.acc[G + i];
    if (a.out_fx) a.out_fx[i] = fx;
    if (a.out_p) a.out_p[i] = static_cast<double>(static_cast<long long>(fx)) * 0x1p-12;
  }
}

}  // namespace grp
}  // namespace kacc

extern "C" {

int kacc_group_sums(kacc_ctx *ctx, kacc_kind kind, const kacc_top_rows *rows, const uint32_t *group, uint32_t n_groups,
                    const uint32_t *node_mask, uint32_t *out_count, uint64_t *out_energy, uint64_t *out_power_fx,
                    double *out_power, uint32_t *out_dropped, void *stream) {
  using namespace kacc::grp;
  const char *fn = "kacc_group_sums";
  if (!ctx) return KACC_EINVAL;
  Args a{};
  int rc = kacc::rows::resolve_kind(ctx, fn, kind);
  if (rc != KACC_OK) return rc;
  if (!rows) return kacc_fail(ctx, KACC_EINVAL, "%s: NULL argument", fn);
  if ((rc = kacc::rows::check_groups(ctx, fn, n_groups)) != KACC_OK) return rc;
  if ((rc = kacc::rows::resolve(ctx, fn, kind, rows, node_mask, &a.v)) != KACC_OK) return rc;
  if (rows->n_rows && !group) return kacc_fail(ctx, KACC_EINVAL, "%s: NULL row array", fn);
  if (!out_count && !out_energy && !out_power_fx && !out_power && !out_dropped)
    return kacc_fail(ctx, KACC_EINVAL, "%s: no output array", fn);
  kacc::rows::Call call(ctx, fn);
  if ((rc = call.open(stream)) != KACC_OK) return rc;
  hipStream_t st = call.st;

  const uint32_t Z = a.v.Z, W = 1u + 2u * Z;
  a.tiles = a.v.n_nodes ? kacc::rows::tiles_of(a.v.n_rows, kTile) : 0u;  // without a node no row is listed
  a.group = group;
  a.n_groups = n_groups;
  a.out_count = out_count;
  a.out_dropped = out_dropped;
  a.out_e = out_energy;
  a.out_fx = out_power_fx;
  a.out_p = out_power;
  a.err = ctx->d_err;

  // the grid: replicated bins (an odd stride: the copies of a bin fall into different banks) while
  // they fit the small LDS size, else one copy in the large one, else passes over group ranges
  const kacc::plan::Bins b = kacc::plan::group_bins(n_groups, Z);
  const bool small = b.regime == kacc::plan::kSmall;
  a.copies = b.copies;
  a.copy_stride = small ? (n_groups * W) | 1u : b.passes > 1 ? 0u : n_groups * W;
  a.passes = b.passes;
  a.bins = b.bins;
  a.splits = kacc::plan::plan_splits(b, a.tiles, kacc::rows::tiles_of(a.v.n_rows, kPassTile));

  // temporaries, stream ordered: the accumulator, the node flags and, for passes, the row words
  // and nodes
  const uint64_t row_words = a.passes > 1 && a.tiles ? a.v.n_rows : 0;
  kacc::plan::Layout tmp;
  tmp.add(&a.acc, static_cast<uint64_t>(n_groups) * W, true);
  tmp.add(&a.v.nflags, a.v.n_nodes);
  for (uint32_t **p : {&a.row_word, &a.row_node}) tmp.add(p, row_words);
  if ((rc = call.alloc(tmp)) != KACC_OK) return rc;

  const dim3 block(kThreads);
  if (a.v.n_nodes) kacc::rows::launch_node_prep<kThreads>(a.v, a.err, kErrGroup, nullptr, st);
  if (a.tiles) {
    kacc::rows::dispatch_zones(Z, [&](auto z) {
      if (a.passes > 1) {
        KACC_LAUNCH(rows_kernel, dim3(a.tiles), block, 0, st, a);
        KACC_LAUNCH(pass_kernel<z()>, dim3(a.passes * a.splits), block, 0, st, a);
      } else if (small) {
        KACC_LAUNCH((bin_kernel<z(), kSmallWords>), dim3(a.splits), block, 0, st, a);
      } else {
        KACC_LAUNCH((bin_kernel<z(), kBigWords>), dim3(a.splits), block, 0, st, a);
      }
    });
  }
  const uint64_t words = static_cast<uint64_t>(n_groups) * Z;
  KACC_LAUNCH(finish_kernel, dim3(static_cast<uint32_t>((words + kThreads - 1) / kThreads)), block, 0, st, a);
  return call.finish();
}

}  // extern "C"
