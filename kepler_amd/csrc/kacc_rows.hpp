// The rows of an interval batch seen tile by tile (device helpers shared by kacc_select.hip,
// kacc_group.hip and kacc_hist.hip; not part of the public ABI): the per-node flag word - is the node listed, and
// which zones passed the guard of a derived power - and the search that finds a row's node in
// row_off, so that workgroups tile the batch rows whatever the node sizes.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kacc_derive.hpp"

namespace kacc {
namespace rows {

constexpr uint32_t kListed = 1u << 31;  // node flag word: bit z = zone z passed the guard
static_assert(KACC_MAX_ZONES < 31, "the zones' guard bits and kListed share a word");

// Node n's flag word, evaluated ONCE per node, for the node that lists the rows: kListed unless
// the mask unlists it, its status flags a read error or its row range is not inside the batch
// (bad_range: the caller raises its error bit), and for a derived power the guard of each zone
// (process.go:124).
__device__ __forceinline__ uint32_t node_flags(const uint32_t *row_off, const uint32_t *node_status,
                                               const uint32_t *node_mask, const ProcDerive &pd, uint32_t derived,
                                               uint32_t Z, uint32_t n_rows, uint32_t n, bool &bad_range) {
  const uint32_t r0 = row_off[n], r1 = row_off[n + 1];
  const uint32_t status = node_status ? node_status[n] : 0u;
  const uint32_t listed = node_mask ? node_mask[n] : 1u;
  uint32_t f = 0;
  if (derived) {  // uniform
    const double cd = pd.cpu_delta[n];
    for (uint32_t z = 0; z < Z; ++z) {
      const uint64_t i = static_cast<uint64_t>(n) * Z + z;
      const bool live = !(pd.active_energy[i] == 0 || !(cd != 0) || !(pd.active_power[i] != 0));
      f |= static_cast<uint32_t>(live) << z;
    }
  }
  bad_range = r0 > r1 || r1 > n_rows;
  if (!bad_range && listed && !(status & KACC_NODE_READ_ERROR)) f |= kListed;
  return f;
}

// One round of a wave-wide 64-ary search for the smallest n in [lo, hi] with off[n + 1] > x
// (kacc_tracker.hip's, over the u32 row offsets): one round trip, the range shrinks 64-fold.
__device__ __forceinline__ void node_search_round(const uint32_t *off, uint32_t x, uint32_t lane, uint32_t &lo,
                                                  uint32_t &hi) {
  const uint64_t st = (hi - lo) / 64u + 1u;
  const uint64_t q = min(lo + lane * st + (st - 1), static_cast<uint64_t>(hi));
  const uint64_t m = __ballot(off[q + 1] > x);
  const uint64_t b = lo + (m ? static_cast<uint32_t>(__builtin_ctzll(m)) : 63u) * st;
  const uint32_t nlo = static_cast<uint32_t>(min(b, static_cast<uint64_t>(hi)));
  const uint32_t nhi = static_cast<uint32_t>(min(b + (st - 1), static_cast<uint64_t>(hi)));
  lo = __builtin_amdgcn_readfirstlane(nlo);
  hi = __builtin_amdgcn_readfirstlane(nhi);
}

struct TileNodes {  // the nodes of the tile's first and last row, and the steps between them
  uint32_t first, last, steps;
};
// The nodes of tile `tile` of `tile_rows` batch rows (tile * tile_rows < n_rows, n_nodes > 0).
__device__ __forceinline__ TileNodes tile_nodes(const uint32_t *row_off, uint32_t n_nodes, uint32_t n_rows,
                                                uint32_t tile, uint32_t tile_rows, uint32_t lane) {
  const uint32_t x0 = tile * tile_rows;  // < n_rows
  const uint32_t x1 = static_cast<uint32_t>(min(static_cast<uint64_t>(x0) + tile_rows, static_cast<uint64_t>(n_rows)) - 1);
  uint32_t la = 0, ha = n_nodes - 1, lb = 0, hb = n_nodes - 1;
  while (ha > la || hb > lb) {  // the two searches' loads share a round trip
    node_search_round(row_off, x0, lane, la, ha);
    node_search_round(row_off, x1, lane, lb, hb);
  }
  TileNodes t;
  t.first = la;
  t.last = max(la, lb);
  const uint32_t span = t.last - t.first;
  t.steps = span ? 32u - static_cast<uint32_t>(__builtin_clz(span)) : 0u;  // ceil(log2(span + 1))
  return t;
}
// One step of a lane's own search between the tile's nodes: the smallest n with
// row_off[n + 1] > r (empty nodes are stepped over).  The load is unconditional.
__device__ __forceinline__ void node_step(const uint32_t *row_off, uint32_t r, uint32_t &lo, uint32_t &hi) {
  const uint32_t mid = (lo + hi) >> 1;
  const bool up = row_off[mid + 1] > r, open = lo < hi;
  hi = (open && up) ? mid : hi;
  lo = (open && !up) ? mid + 1 : lo;
}

}  // namespace rows
}  // namespace kacc
