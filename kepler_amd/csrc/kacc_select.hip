// Running workloads above a threshold, selected on the device.
//
// No reference counterpart: Kepler exports every running workload and leaves the cut to
// PromQL; a fleet engine exports "every process above 1 W".  An order-preserving filter of
// the rows of the caller's last interval batch (one workload kind): row r is selected iff
// key(value(r)) >= key(threshold), value and key by the shared row layer (kacc_rows.hpp), and
// the selected rows leave in batch row order with their slot, node and Z-word energy / power
// records, dense, with per-node offsets.
//
// count -> scan -> scatter, no workgroup waits on another and no atomic places an item:
//   node_prep     the shared layer's: one flag word per node; it also clears cnt[tiles]
//   count         one workgroup per tile of kTile batch rows, located by the shared layer's
//                 tile prelude (balanced whatever the node sizes).  Evaluates the predicate,
//                 leaves one selection bit per row (a wave's ballot is the 64 rows' word) and
//                 the tile's count
//   scan          kacc_internal_scan_u64 over the tile counts
//   scatter       one workgroup per tile: reads the tile's 32 mask words instead of evaluating
//                 the predicate again; an item's position is the tile's offset + the popcounts
//                 in front of it.  A wave copies the Z-word records of a word's items as one
//                 contiguous output range (16-B accesses for an even Z and aligned outputs)
//   node_off      one thread per node: the items in front of the node's first row, out of the
//                 tile offsets and the mask words
// Every index is clamped (the shared layer's rules), so no batch faults.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kacc_derive.hpp"
#include "kacc_internal.hpp"
#include "kacc_rows.hpp"

namespace kacc {
namespace sel {

constexpr uint32_t kThreads = 256, kWaves = kThreads / 64;
constexpr uint32_t kPer = 8;                   // 64-row words per wave
constexpr uint32_t kWords = kWaves * kPer;     // mask words per tile (<= 64: one per lane)
constexpr uint32_t kTile = kWords * 64;        // rows per tile
constexpr uint32_t kErrSelect = 1u << 12;      // more items than item_cap, a slot past the capacity,
                                               // a row range outside the batch
using rows::kDerived, rows::kEnergy, rows::kStored;  // the table of the predicate

struct Args {
  rows::View v;
  // the predicate's table
  const uint64_t *words;  // energy / stored power words of `zone`: words[slot * v.tab_stride]
  uint32_t zone;
  uint64_t thr_key;
  uint32_t tiles;
  // scratch
  uint64_t *mask;    // [tiles * kWords] bit (r & 63) of word r / 64: row r is selected
  uint64_t *cnt;     // [tiles + 1] selected rows per tile, cnt[tiles] = 0
  uint64_t *off;     // [tiles + 1] their exclusive scan: off[tiles] = the total
  // the outputs
  uint32_t item_cap;
  uint32_t *node_off, *out_row, *out_slot, *out_node;
  uint64_t *out_e, *out_p;
  uint32_t *err;
};

template <int kSrc>
__global__ __launch_bounds__(kThreads) void count_kernel(const Args a) {
  __shared__ uint32_t s_cnt[kWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, tile = blockIdx.x;
  const uint32_t word0 = wave * kPer;  // the wave's kPer consecutive words of the tile
  rows::Located<kPer> t;
  rows::locate<kPer>(a.v, nullptr, tile, kTile, lane, wave, t);
#pragma unroll
  for (uint32_t u = 0; u < kPer; ++u) rows::check_row(a.v, 1u, t, u);
  uint32_t c = 0;
#pragma unroll
  for (uint32_t u = 0; u < kPer; ++u) {
    uint64_t v = 0;
    if (a.v.cap != 0)  // uniform
      v = rows::value_bits<kSrc>(a.words, a.v.tab_stride, a.v.pd, a.v.Z, a.zone, t.sl[u], t.node[u], t.f[u]);
    const uint64_t key = kSrc == kEnergy ? v : rows::power_key(v);
    const uint64_t m = __ballot(t.ok[u] && key >= a.thr_key);
    if (lane == 0) a.mask[static_cast<uint64_t>(tile) * kWords + word0 + u] = m;
    c += static_cast<uint32_t>(__popcll(m));
  }
  if (t.bad) atomicOr(a.err, kErrSelect);  // left out
  if (lane == 0) s_cnt[wave] = c;
  __syncthreads();
  if (tid == 0) {
    uint32_t sum = 0;
    for (uint32_t i = 0; i < kWaves; ++i) sum += s_cnt[i];
    a.cnt[tile] = sum;
  }
}

using u64x2 = __attribute__((ext_vector_type(2))) unsigned long long;

// kDer: the power is derived (ratio[slot] · ActivePower[node], the node's guard flag), else the
// stored record.  kW: words per lane and copy (2: 16-B loads and stores; an even Z, aligned outputs).
template <bool kDer, uint32_t kW>
__global__ __launch_bounds__(kThreads) void scatter_kernel(const Args a) {
  __shared__ uint32_t s_slot[kWaves][64], s_node[kWaves][64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, tile = blockIdx.x;
  const rows::View &v = a.v;
  const uint32_t Z = v.Z;
  const uint64_t limit = min(a.off[a.tiles], static_cast<uint64_t>(a.item_cap));
  const uint64_t tbase = a.off[tile];
  if (tbase >= limit) return;  // workgroup-uniform: nothing of this tile fits (or it is empty and last)
  // the tile's words, one per lane, and their exclusive popcount scan
  const uint64_t mw = a.mask[static_cast<uint64_t>(tile) * kWords + min(lane, kWords - 1)];
  const uint32_t pc = lane < kWords ? static_cast<uint32_t>(__popcll(mw)) : 0u;
  uint32_t inc = pc;
#pragma unroll
  for (uint32_t d = 1; d < kWords; d <<= 1) {
    const uint32_t t = __shfl_up(inc, d, 64);
    inc += lane >= d ? t : 0u;
  }
  const uint32_t excl = inc - pc;
  const rows::TileNodes tn = rows::tile_nodes(v.row_off, v.n_nodes, v.n_rows, tile, kTile, lane);
  const uint32_t last_row = v.n_rows - 1;

  for (uint32_t u = 0; u < kPer; ++u) {
    const uint32_t j = wave * kPer + u;
    const uint64_t m = __shfl(mw, static_cast<int>(j), 64);
    const uint64_t base = tbase + __shfl(excl, static_cast<int>(j), 64);
    const uint32_t c = static_cast<uint32_t>(__popcll(m));
    if (c == 0 || base >= limit) continue;  // wave-uniform
    const uint64_t rr = static_cast<uint64_t>(tile) * kTile + j * 64u + lane;
    const uint32_t r = static_cast<uint32_t>(min(rr, static_cast<uint64_t>(last_row)));
    const uint32_t sw = v.slot[r] & KACC_SLOT_MASK;
    const uint32_t sl = sw < v.cap ? sw : 0u;  // a selected row's slot is below the capacity (the count pass)
    uint32_t lo = tn.first, hi = tn.last;
    for (uint32_t s = 0; s < tn.steps; ++s) rows::node_step(v.row_off, r, lo, hi);
    const bool sel = (m >> lane) & 1ull;
    const uint32_t rank = static_cast<uint32_t>(__popcll(m & ((1ull << lane) - 1ull)));
    const uint64_t i = base + rank;
    if (sel) {
      s_slot[wave][rank] = sl;
      s_node[wave][rank] = lo;
      if (i < limit) {
        if (a.out_row) a.out_row[i] = r;
        if (a.out_slot) a.out_slot[i] = sl;
        if (a.out_node) a.out_node[i] = lo;
      }
    }
    rows::wave_lds_fence();
    // the c items' records are one contiguous output range of c Z words: lane l takes words
    // kW (64 k + l) .. + kW, each word's slot and node from its item's entry
    const uint32_t words = static_cast<uint32_t>(min(static_cast<uint64_t>(c), limit - base)) * Z;
    const uint64_t o0 = base * Z;
    for (uint32_t k = 0; k * 64u * kW < words; ++k) {  // wave-uniform
      const uint32_t wd = (k * 64u + lane) * kW;
      const bool valid = wd < words;
      const uint32_t itq = wd / Z;
      const uint32_t it = valid ? itq : 0u, z = valid ? wd - itq * Z : 0u;  // kW = 2: z is even and Z is
      const uint64_t s = s_slot[wave][it];
      const uint64_t nd = s_node[wave][it];
      if (a.out_e) {
        const uint64_t *src = v.tab_e + s * v.tab_stride + z;
        if constexpr (kW == 2) {
          const u64x2 e = *reinterpret_cast<const u64x2 *>(src);
          if (valid) *reinterpret_cast<u64x2 *>(a.out_e + o0 + wd) = e;
        } else {
          const uint64_t e = *src;
          if (valid) a.out_e[o0 + wd] = e;
        }
      }
      if (a.out_p) {
        uint64_t p[kW];
        if constexpr (kDer) {
          const double ratio = v.pd.ratio[s];
          const uint32_t f = v.nflags[nd];
          const double *aP = v.pd.active_power + nd * Z + z;
          double ap[kW];
          if constexpr (kW == 2) {
            const u64x2 t = *reinterpret_cast<const u64x2 *>(aP);
            ap[0] = __longlong_as_double(static_cast<long long>(t.x));
            ap[1] = __longlong_as_double(static_cast<long long>(t.y));
          } else {
            ap[0] = *aP;
          }
#pragma unroll
          for (uint32_t q = 0; q < kW; ++q)
            p[q] = rows::derived_bits(f, z + q, ratio, ap[q]);
        } else {
          const uint64_t *src = v.tab_p + s * v.tab_stride + z;
          if constexpr (kW == 2) {
            const u64x2 t = *reinterpret_cast<const u64x2 *>(src);
            p[0] = t.x;
            p[1] = t.y;
          } else {
            p[0] = *src;
          }
        }
        if (valid) {
          if constexpr (kW == 2) {
            u64x2 t;
            t.x = p[0];
            t.y = p[1];
            *reinterpret_cast<u64x2 *>(a.out_p + o0 + wd) = t;
          } else {
            a.out_p[o0 + wd] = p[0];
          }
        }
      }
    }
    rows::wave_lds_fence();  // the next word's entries overwrite these
  }
}

// node_off[n] = the items in front of node n's first row; node_off[n_nodes] = the total.
__global__ __launch_bounds__(kThreads) void node_off_kernel(const Args a) {
  const uint32_t n = blockIdx.x * kThreads + threadIdx.x;
  const uint64_t total = a.off[a.tiles];
  // item_cap 0 is the sizing call
  if (n == 0 && total > a.item_cap && a.item_cap) atomicOr(a.err, kErrSelect);
  if (n > a.v.n_nodes) return;
  uint64_t pos = total;
  if (a.tiles) {  // uniform
    const uint32_t r = min(a.v.row_off[min(n, a.v.n_nodes)], a.v.n_rows);  // n = n_nodes: the batch's end
    const uint32_t rc = min(r, a.v.n_rows - 1);
    const uint32_t tile = rc / kTile, j = (rc % kTile) / 64u, b = rc & 63u;
    uint64_t p = a.off[tile];
#pragma unroll 8
    for (uint32_t i = 0; i < kWords; ++i) {
      const uint64_t m = a.mask[static_cast<uint64_t>(tile) * kWords + i];
      const uint64_t take = i < j ? ~0ull : (i == j ? (1ull << b) - 1ull : 0ull);
      p += static_cast<uint32_t>(__popcll(m & take));
    }
    pos = r < a.v.n_rows ? p : total;
  }
  a.node_off[n] = static_cast<uint32_t>(pos);  // <= n_rows
}

}  // namespace sel
}  // namespace kacc

extern "C" {

int kacc_select_above(kacc_ctx *ctx, kacc_table t, uint32_t zone, uint64_t threshold, const kacc_top_rows *rows,
                      const uint32_t *node_mask, uint32_t item_cap, uint32_t *node_off, uint32_t *out_row,
                      uint32_t *out_slot, uint32_t *out_node, uint64_t *out_energy, double *out_power,
                      void *stream) {
  using namespace kacc::sel;
  const char *fn = "kacc_select_above";
  if (!ctx) return KACC_EINVAL;
  kacc::rows::Table tab;
  Args a{};
  int rc = kacc::rows::resolve_table(ctx, fn, t, zone, &tab);
  if (rc != KACC_OK) return rc;
  if (!rows || !node_off) return kacc_fail(ctx, KACC_EINVAL, "%s: NULL argument", fn);
  if ((rc = kacc::rows::resolve(ctx, fn, tab.kind, rows, node_mask, &a.v)) != KACC_OK) return rc;
  if (item_cap && !out_row && !out_slot && !out_node && !out_energy && !out_power)
    return kacc_fail(ctx, KACC_EINVAL, "%s: item_cap %u and no output array", fn, item_cap);
  if (rows->n_nodes == 0) {  // no node lists a row: no launch, and a pending launch timing stays pending
    hipStream_t st = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
    KACC_HIP(ctx, hipSetDevice(ctx->device));
    KACC_HIP(ctx, hipMemsetAsync(node_off, 0, sizeof(uint32_t), st));
    return KACC_OK;
  }
  kacc::rows::Call call(ctx, fn);
  if ((rc = call.open(stream)) != KACC_OK) return rc;
  hipStream_t st = call.st;

  const uint32_t Z = a.v.Z;
  a.words = tab.words;
  a.zone = zone;
  a.thr_key = tab.power ? kacc::rows::power_key(threshold) : threshold;  // NaN: 0, every listed row
  a.tiles = kacc::rows::tiles_of(a.v.n_rows, kTile);
  a.item_cap = item_cap;
  a.node_off = node_off;
  a.out_row = out_row;
  a.out_slot = out_slot;
  a.out_node = out_node;
  a.out_e = out_energy;
  a.out_p = reinterpret_cast<uint64_t *>(out_power);
  a.err = ctx->d_err;

  // temporaries, stream ordered: the mask, the tile counts, their scan, the scan's tile sums, the node flags
  const uint64_t n = a.tiles + 1ull, scan_tiles = kacc_internal_scan_tiles(n);
  const uint64_t mask_words = static_cast<uint64_t>(a.tiles) * kWords;
  uint64_t *tile_sum = nullptr;
  kacc::plan::Layout tmp;
  tmp.add(&a.mask, mask_words);
  for (uint64_t **p : {&a.cnt, &a.off}) tmp.add(p, n);
  tmp.add(&tile_sum, scan_tiles);
  tmp.add(&a.v.nflags, a.v.n_nodes);
  if ((rc = call.alloc(tmp)) != KACC_OK) return rc;

  const dim3 node_grid(static_cast<uint32_t>((a.v.n_nodes + 1ull + kThreads - 1) / kThreads)), block(kThreads);
  kacc::rows::launch_node_prep<kThreads>(a.v, a.err, kErrSelect, a.cnt + a.tiles, st);
  if (a.tiles)
    kacc::rows::dispatch_src(tab.src, [&](auto s) { KACC_LAUNCH(count_kernel<s()>, dim3(a.tiles), block, 0, st, a); });
  if ((rc = kacc_internal_scan_u64(ctx, a.cnt, n, tile_sum, a.off, st)) != KACC_OK) return rc;
  if (a.tiles && item_cap) {
    // 16-B copies for an even Z when the caller's arrays allow them (the tables are hipMalloc'ed)
    const bool wide = Z % 2 == 0 &&
                      ((reinterpret_cast<uintptr_t>(out_energy) | reinterpret_cast<uintptr_t>(out_power)) & 15u) == 0;
    if (a.v.derived && wide)
      KACC_LAUNCH((scatter_kernel<true, 2>), dim3(a.tiles), block, 0, st, a);
    else if (a.v.derived)
      KACC_LAUNCH((scatter_kernel<true, 1>), dim3(a.tiles), block, 0, st, a);
    else if (wide)
      KACC_LAUNCH((scatter_kernel<false, 2>), dim3(a.tiles), block, 0, st, a);
    else
      KACC_LAUNCH((scatter_kernel<false, 1>), dim3(a.tiles), block, 0, st, a);
  }
  KACC_LAUNCH(node_off_kernel, node_grid, block, 0, st, a);
  return call.finish();
}

}  // extern "C"
