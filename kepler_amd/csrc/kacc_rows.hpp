// The rows of an interval batch for the workload row queries - kacc_top.hip, kacc_select.hip,
// kacc_group.hip, kacc_hist.hip, kacc_quant.hip, kacc_gtop.hip, kacc_window.hip (DESIGN §4.10b;
// device and host helpers, not part of the public ABI).  All seven read the rows of the caller's
// last interval batch (kacc_top_rows) for one workload kind and ask the same things: is the row
// listed, is its slot valid, what is its value (an energy word, a stored pod power, or the derived
// ratio[slot] · ActivePower[node] under the node's guard) or its Z-word record.  Here, once: the
// value rules, the row view, the per-node flag word and its kernel, the tile-to-node search, the
// tile prelude that locates a lane's rows, the pass queue, the host resolver of a call's kind and
// rows, and the host's call layer: the call scope with its scratch, the source and zone
// dispatch and the small helpers (the scratch layout and the LDS plan are kacc_plan.hpp's).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>
#include <optional>
#include <type_traits>

#include "kacc_derive.hpp"
#include "kacc_internal.hpp"
#include "kacc_plan.hpp"

namespace kacc {
namespace rows {

// ---- values -------------------------------------------------------------------------------

enum Src { kEnergy = 0, kStored = 1, kDerived = 2 };  // where a row's value comes from

constexpr uint32_t kListed = 1u << 31;  // node flag word: bit z = zone z passed the guard
static_assert(KACC_MAX_ZONES < 31, "the zones' guard bits and kListed share a word");
constexpr uint64_t kFxLimit = (1023ull + 50ull) << 52;  // the bits of 2^50: |p| at or past it has no fx
using plan::kCus, plan::kMaxCopies;   // the persistent grids and the LDS copies of the group queries
constexpr uint32_t kQueue = 128;      // a wave's queued rows in a pass
constexpr uint32_t kPassPer = 16;     // row words per lane and step of a pass

// The order rule's key of a power (header): NaN lowest, the zeros equal, else the IEEE order.
__host__ __device__ __forceinline__ uint64_t power_key(uint64_t b) {
  const uint32_t hi = static_cast<uint32_t>(b >> 32), lo = static_cast<uint32_t>(b);
  const uint32_t mag = hi & 0x7fffffffu;
  if (mag > 0x7ff00000u || (mag == 0x7ff00000u && lo != 0)) return 0;  // NaN
  if ((mag | lo) == 0) return 0x8000000000000000ull;                   // ±0
  return (hi >> 31) ? ~b : (b | 0x8000000000000000ull);
}
// The value bits a non-NaN key came from: an energy's are the key itself, a power's come back
// through this inverse of power_key (either zero as +0.0).
__host__ __device__ __forceinline__ uint64_t power_key_bits(uint64_t key) {
  return (key >> 63) ? (key & 0x7fffffffffffffffull) : ~key;
}
// fx(p) of the header for the f64 with these bits; keep: finite and |p| < 2^50, else fx is 0.
__device__ __forceinline__ uint64_t power_fx(uint64_t bits, bool &keep) {
  keep = (bits & 0x7fffffffffffffffull) < kFxLimit;
  const double p = __longlong_as_double(static_cast<long long>(keep ? bits : 0ull));
  return static_cast<uint64_t>(static_cast<long long>(p * 4096.0));  // exact product, truncated toward zero
}
// The bits of a derived power in zone z: ratio · ActivePower under bit z of the node's flag word.
__device__ __forceinline__ uint64_t derived_bits(uint32_t f, uint32_t z, double ratio, double aP) {
  return static_cast<uint64_t>(__double_as_longlong(((f >> z) & 1u) ? ratio * aP : 0.0));
}
__device__ __forceinline__ void lds_add(uint64_t *p, uint64_t v) {
  atomicAdd(reinterpret_cast<unsigned long long *>(p), static_cast<unsigned long long>(v));
}
__device__ __forceinline__ void wave_lds_fence() {  // a wave's LDS writes before its reads
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- the row view --------------------------------------------------------------------------

struct View {  // one call's rows and the records of their kind
  uint32_t n_nodes, n_rows;
  const uint32_t *row_off, *slot, *node_status, *node_mask;
  uint32_t *nflags;  // [n_nodes] scratch: the nodes' flag words (node_prep_kernel)
  uint64_t cap;      // the kind's slot capacity
  const uint64_t *tab_e, *tab_p;  // the kind's energy table; the stored power (pods) or NULL
  uint32_t tab_stride;            // Z, or 2Z for the pod records
  ProcDerive pd;                  // derived power
  uint32_t Z, derived;            // derived: the kind's power is (every kind but the pods)
};

__host__ __device__ __forceinline__ uint32_t tiles_of(uint32_t n_rows, uint32_t tile_rows) {
  return static_cast<uint32_t>((static_cast<uint64_t>(n_rows) + tile_rows - 1) / tile_rows);
}

// The value bits of a row for kSrc: words[slot * stride] (the table's words of the zone), or the
// derived power of (slot, zone) on `node` whose flag word is f.  sl is the clamped slot.
template <int kSrc>
__device__ __forceinline__ uint64_t value_bits(const uint64_t *words, uint32_t stride, const ProcDerive &pd, uint32_t Z,
                                               uint32_t zone, uint32_t sl, uint32_t node, uint32_t f) {
  if constexpr (kSrc == kDerived) {
    const double ratio = pd.ratio[sl];
    return derived_bits(f, zone, ratio, pd.active_power[static_cast<uint64_t>(node) * Z + zone]);
  } else {
    return words[static_cast<uint64_t>(sl) * stride];
  }
}

// Node n's flag word, evaluated ONCE per node, for the node that lists the rows: kListed unless
// the mask unlists it, its status flags a read error or its row range is not inside the batch
// (bad_range: the caller raises its error bit), and for a derived power the guard of each zone
// (process.go:124).
__device__ __forceinline__ uint32_t node_flags(const View &v, uint32_t n, bool &bad_range) {
  const uint32_t r0 = v.row_off[n], r1 = v.row_off[n + 1];
  const uint32_t status = v.node_status ? v.node_status[n] : 0u;
  const uint32_t listed = v.node_mask ? v.node_mask[n] : 1u;
  uint32_t f = 0;
  if (v.derived) {  // uniform
    const double cd = v.pd.cpu_delta[n];
    for (uint32_t z = 0; z < v.Z; ++z) {
      const uint64_t i = static_cast<uint64_t>(n) * v.Z + z;
      const bool live = !(v.pd.active_energy[i] == 0 || !(cd != 0) || !(v.pd.active_power[i] != 0));
      f |= static_cast<uint32_t>(live) << z;
    }
  }
  bad_range = r0 > r1 || r1 > v.n_rows;
  if (!bad_range && listed && !(status & KACC_NODE_READ_ERROR)) f |= kListed;
  return f;
}
// One thread per node: the flag words.  A bad row range raises err_bit (the node is left out);
// `zero`, when not NULL, is a scratch word the caller wants cleared by this launch (then the
// grid covers n_nodes + 1 threads, so that it runs without a node too).
template <uint32_t kThreads>
__global__ __launch_bounds__(kThreads) void node_prep_kernel(const View v, uint32_t *err, uint32_t err_bit,
                                                             uint64_t *zero) {
  const uint32_t n = blockIdx.x * kThreads + threadIdx.x;
  if (n == 0 && zero) *zero = 0;
  if (n >= v.n_nodes) return;
  bool bad_range;
  const uint32_t f = node_flags(v, n, bad_range);
  if (bad_range) atomicOr(err, err_bit);  // left out
  v.nflags[n] = f;
}

// ---- a row's node --------------------------------------------------------------------------

// One round of a wave-wide 64-ary search for the smallest n in [lo, hi] with off[n + 1] > x
// (the tracker read's search, here over the u32 row offsets): one round trip, the range shrinks 64-fold.
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

// ---- the tile prelude ----------------------------------------------------------------------

// The id check of a row: true when g is a group; bad_id: neither a group nor KACC_GROUP_NONE
// (a listed row with it is left out and reported).
__device__ __forceinline__ bool group_ok(uint32_t g, uint32_t n_groups, bool &bad_id) {
  const bool gin = g < n_groups;
  bad_id = !gin && g != KACC_GROUP_NONE;
  return gin;
}

template <uint32_t kPer>
struct Located {  // a lane's kPer rows of a tile: rows (wave * kPer + u) * 64 + lane of the tile
  bool in_batch[kPer];                     // else the row is clamped to the batch's last row
  bool ok[kPer];                           // listed - in the batch, in a listed node that contains it - with
                                           // a slot below the capacity and an id below n_groups
  uint32_t r[kPer], node[kPer], f[kPer];   // the row, its node, the node's flag word
  uint32_t w[kPer], sl[kPer], g[kPer];     // the slot word, the slot (clamped to slot 0), the group id
  bool bad;  // a listed row of this lane has a slot or an id out of range: it is left out, the
             // caller raises its error bit
};
// Locates the rows of tile `tile` of tile_rows = waves * kPer * 64 batch rows: r, in_batch, w, g
// and node; check_row completes a row.  No load sits behind a data-dependent branch: a row past
// the batch is clamped to its last row, a bad slot to slot 0, a node by the search's range.
// The statement order - all slot loads, then all search steps, then (the caller's loop over
// check_row) all node reloads - keeps a lane's kPer loads of one kind in flight together.
// `group` NULL: every row in group 0 (uniform).
template <uint32_t kPer>
__device__ __forceinline__ void locate(const View &v, const uint32_t *group, uint32_t tile, uint32_t tile_rows,
                                       uint32_t lane, uint32_t wave, Located<kPer> &t) {
  const TileNodes tn = tile_nodes(v.row_off, v.n_nodes, v.n_rows, tile, tile_rows, lane);
  const uint64_t row0 = static_cast<uint64_t>(tile) * tile_rows + wave * (kPer * 64u) + lane;
  const uint32_t last_row = v.n_rows - 1;
  uint32_t hi[kPer];
#pragma unroll
  for (uint32_t u = 0; u < kPer; ++u) {
    const uint64_t rr = row0 + u * 64u;
    t.in_batch[u] = rr <= last_row;
    t.r[u] = static_cast<uint32_t>(min(rr, static_cast<uint64_t>(last_row)));
    t.w[u] = v.slot[t.r[u]];
    t.g[u] = 0u;
    t.node[u] = tn.first;
    hi[u] = tn.last;
  }
  if (group) {  // uniform, tested once: the id loads join the slot loads in flight
#pragma unroll
    for (uint32_t u = 0; u < kPer; ++u) t.g[u] = group[t.r[u]];
  }
  for (uint32_t s = 0; s < tn.steps; ++s) {  // workgroup-uniform
#pragma unroll
    for (uint32_t u = 0; u < kPer; ++u) node_step(v.row_off, t.r[u], t.node[u], hi[u]);
  }
  t.bad = false;
}
// Row u of a located tile: the node's range and flag word, is the row listed, its slot, its id.
template <uint32_t kPer>
__device__ __forceinline__ void check_row(const View &v, uint32_t n_groups, Located<kPer> &t, uint32_t u) {
  const uint32_t n = t.node[u];
  const uint32_t r0 = v.row_off[n], r1 = v.row_off[n + 1];
  t.f[u] = v.nflags[n];
  const bool listed = t.in_batch[u] && r0 <= t.r[u] && t.r[u] < r1 && (t.f[u] & kListed);
  const uint32_t s = t.w[u] & KACC_SLOT_MASK;
  const bool in = s < v.cap;
  bool bad_id;
  const bool gin = group_ok(t.g[u], n_groups, bad_id);
  t.bad = t.bad || (listed && (!in || bad_id));
  t.ok[u] = listed && in && gin;
  t.sl[u] = in ? s : 0u;
}

// ---- the pass queue ------------------------------------------------------------------------

// A pass's walk over the row words of a classified batch (persistent workgroup `split` of
// `splits`, kThreads threads, q: the wave's kQueue LDS words).  About one row word in `passes`
// is the pass's - mine(word) - so a wave first queues its rows (ballot and popcount) and hands
// them to drain(n) 64 at a time: q[0 .. n), n <= 64, one row per lane, so the loads of 64 rows
// are in flight together.
template <uint32_t kThreads, class Mine, class Drain>
__device__ __forceinline__ void pass_queue(const uint32_t *row_word, uint32_t n_rows, uint32_t split, uint32_t splits,
                                           uint32_t lane, uint32_t wave, uint32_t *q, Mine mine, Drain drain) {
  constexpr uint32_t kPassTile = kThreads * kPassPer;
  const uint32_t last_row = n_rows - 1, pass_tiles = tiles_of(n_rows, kPassTile);
  uint32_t qn = 0;  // wave-uniform: the queued rows, < 64 between steps
  for (uint32_t tile = split; tile < pass_tiles; tile += splits) {  // workgroup-uniform
    const uint64_t row0 = static_cast<uint64_t>(tile) * kPassTile + wave * (kPassPer * 64u) + lane;
    uint32_t word[kPassPer];
#pragma unroll
    for (uint32_t u = 0; u < kPassPer; ++u)  // a row past the batch is clamped to its last row
      word[u] = row_word[static_cast<uint32_t>(min(row0 + u * 64u, static_cast<uint64_t>(last_row)))];
#pragma unroll
    for (uint32_t u = 0; u < kPassPer; ++u) {
      const uint64_t rr = row0 + u * 64u;
      const bool in = rr <= last_row && mine(word[u]);
      const uint64_t m = __ballot(in);
      if (m == 0) continue;  // wave-uniform
      if (in) q[qn + static_cast<uint32_t>(__popcll(m & ((1ull << lane) - 1ull)))] = static_cast<uint32_t>(rr);
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
}

// ---- the host's resolver -------------------------------------------------------------------

struct Table {  // a workload table's kind, the Src of its values and its words of the zone
  int kind, src;
  bool power;
  const uint64_t *words;  // words[slot * tab_stride]; pod power: Z words into the record
};
// Front door of the calls that take a table and a zone.
inline int resolve_table(kacc_ctx *ctx, const char *fn, int t, uint32_t zone, Table *tab) {
  switch (t) {
    case KACC_T_PROC_ENERGY: case KACC_T_PROC_POWER: tab->kind = KACC_KIND_PROC; break;
    case KACC_T_CTR_ENERGY: case KACC_T_CTR_POWER: tab->kind = KACC_KIND_CTR; break;
    case KACC_T_VM_ENERGY: case KACC_T_VM_POWER: tab->kind = KACC_KIND_VM; break;
    case KACC_T_POD_ENERGY: case KACC_T_POD_POWER: tab->kind = KACC_KIND_POD; break;
    default: return kacc_fail(ctx, KACC_EINVAL, "%s: table %d is not a workload energy / power table", fn, t);
  }
  if (zone >= ctx->cfg.zones) return kacc_fail(ctx, KACC_EINVAL, "%s: zone %u >= Z = %u", fn, zone, ctx->cfg.zones);
  tab->power = t == KACC_T_PROC_POWER || t == KACC_T_CTR_POWER || t == KACC_T_VM_POWER || t == KACC_T_POD_POWER;
  tab->src = !tab->power ? kEnergy : tab->kind == KACC_KIND_POD ? kStored : kDerived;
  tab->words = static_cast<const uint64_t *>(ctx->tables[t]) + zone;
  return KACC_OK;
}
// Front door of the calls that take a kind.
inline int resolve_kind(kacc_ctx *ctx, const char *fn, int kind) {
  if (kind != KACC_KIND_PROC && kind != KACC_KIND_CTR && kind != KACC_KIND_VM && kind != KACC_KIND_POD)
    return kacc_fail(ctx, KACC_EINVAL, "%s: unknown kind %d", fn, kind);
  return KACC_OK;
}
// The resolver: validates the caller's rows against the context and fills the view with them
// and the records of `kind` (a front door's).  nflags is the caller's scratch, set later.
inline int resolve(kacc_ctx *ctx, const char *fn, int kind, const kacc_top_rows *rows, const uint32_t *node_mask,
                   View *v) {
  if (!rows) return kacc_fail(ctx, KACC_EINVAL, "%s: NULL argument", fn);
  if (rows->n_nodes > ctx->cfg.nodes)
    return kacc_fail(ctx, KACC_EINVAL, "%s: n_nodes %u > the context's %llu nodes", fn, rows->n_nodes,
                     (unsigned long long)ctx->cfg.nodes);
  if (!rows->row_off || (rows->n_rows && !rows->slot)) return kacc_fail(ctx, KACC_EINVAL, "%s: NULL row array", fn);
  const bool pod = kind == KACC_KIND_POD;
  *v = View{};
  v->n_nodes = rows->n_nodes;
  v->n_rows = rows->n_rows;
  v->row_off = rows->row_off;
  v->slot = rows->slot;
  v->node_status = rows->node_status;
  v->node_mask = node_mask;
  v->cap = kind_cap(ctx, kind);
  v->Z = ctx->cfg.zones;
  v->tab_stride = pod ? 2 * v->Z : v->Z;
  v->tab_e = static_cast<const uint64_t *>(ctx->tables[kind_energy_table(kind)]);
  v->tab_p = pod ? static_cast<const uint64_t *>(ctx->tables[KACC_T_POD_POWER]) : nullptr;  // Z words into the record
  v->pd = kacc_derive(ctx, static_cast<kacc_kind>(pod ? KACC_KIND_PROC : kind));
  v->derived = !pod;  // the kind's power, whichever table a call's values come from
  return KACC_OK;
}
// The group count's range, one rule for every call that takes one.
inline int check_groups(kacc_ctx *ctx, const char *fn, uint32_t n_groups) {
  if (n_groups < 1 || n_groups > KACC_GROUP_MAX)
    return kacc_fail(ctx, KACC_EINVAL, "%s: n_groups %u outside 1 .. %u", fn, n_groups, KACC_GROUP_MAX);
  return KACC_OK;
}

// ---- the host's call layer -----------------------------------------------------------------

// One entry point's device work, after its argument checks: open() sets the device, resolves
// the stream, takes the context's pending timing events and drops a stale launch error;
// alloc() makes the call's one scratch allocation and its one memset; finish() turns a launch
// error into the return code.  The scratch is freed, stream ordered, on every path out.
class Call {
 public:
  kacc_ctx *const ctx;
  const char *const fn;
  hipStream_t st = nullptr;

  Call(kacc_ctx *c, const char *f) : ctx(c), fn(f) {}
  ~Call() {
    if (tmp_) (void)hipFreeAsync(tmp_, st);
  }

  int open(void *stream) {
    KACC_HIP(ctx, hipSetDevice(ctx->device));
    st = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
    timing_.emplace(ctx);
    (void)hipGetLastError();  // as everywhere in the library: finish() reports this call's launches alone
    return KACC_OK;
  }
  // The layout's arrays (none: no allocation), at least min_bytes; its pointers are set.
  int alloc(const plan::Layout &l, uint64_t min_bytes = 0) {
    const uint64_t bytes = std::max(l.bytes(), min_bytes);
    if (!bytes) return KACC_OK;
    KACC_HIP(ctx, hipMallocAsync(&tmp_, bytes, st));
    l.bind(tmp_);
    if (l.zeroed() && hipMemsetAsync(tmp_, 0, l.zeroed(), st) != hipSuccess)
      return kacc_fail(ctx, KACC_EHIP, "%s: memset", fn);
    return KACC_OK;
  }
  int finish() {
    return hipGetLastError() != hipSuccess ? kacc_fail(ctx, KACC_EHIP, "%s: launch", fn) : KACC_OK;
  }

 private:
  std::optional<TimingScope> timing_;
  void *tmp_ = nullptr;
};

// f(std::integral_constant<int, kSrc>{}) for the Src of a call's values: one generic lambda
// around the launch of a kernel<kSrc>.
template <class F>
void dispatch_src(int src, F f) {
  if (src == kEnergy)
    f(std::integral_constant<int, kEnergy>{});
  else if (src == kStored)
    f(std::integral_constant<int, kStored>{});
  else
    f(std::integral_constant<int, kDerived>{});
}
// The same for a kernel<kZ>: 4 when that is the zone count (16-byte loads), else 0: any Z.
template <class F>
void dispatch_zones(uint32_t Z, F f) {
  if (Z == 4)
    f(std::integral_constant<uint32_t, 4>{});
  else
    f(std::integral_constant<uint32_t, 0>{});
}

// The launch of the view's node_prep_kernel: one thread per node, and one more when `zero`
// (a scratch word to clear) makes it run without a node too.
template <uint32_t kThreads>
void launch_node_prep(const View &v, uint32_t *err, uint32_t err_bit, uint64_t *zero, hipStream_t st) {
  const uint64_t threads = v.n_nodes + (zero ? 1ull : 0ull);
  KACC_LAUNCH(node_prep_kernel<kThreads>, dim3(static_cast<uint32_t>((threads + kThreads - 1) / kThreads)),
              dim3(kThreads), 0, st, v, err, err_bit, zero);
}

// A tuning knob of the tools' benchmarks: the value of an environment variable, at most `cap`.
inline uint32_t knob(const char *name, uint32_t dflt, uint32_t cap) {
  const char *s = std::getenv(name);
  if (!s || !*s) return dflt;
  return static_cast<uint32_t>(std::min<unsigned long>(std::strtoul(s, nullptr, 10), cap));
}

}  // namespace rows
}  // namespace kacc
