// The host arithmetic of the workload row queries: a call's scratch layout and the
// plan of a group query's LDS bins.  Free of HIP, so that the host compiler alone builds and tests
// it (tests/c/rows_plan.cpp); kacc_rows.hpp puts the device allocation and the launches on top.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <cassert>
#include <cstring>

namespace kacc {
namespace plan {

// ---- the scratch layout ---------------------------------------------------------------------

// The arrays of a call's one scratch allocation, declared in memory order: add(&p, n, zeroed)
// places n elements of *p's type at the next multiple of the element size and remembers p;
// bind(base) points every p into the allocation.  The zeroed arrays come first: [0, zeroed())
// is the call's one memset.  Size, offsets and pointers come from the same declarations.
class Layout {
 public:
  template <class T>
  void add(T **p, uint64_t n, bool zeroed = false) {
    assert(n_ < kMaxArrays && (!zeroed || bytes_ <= ((zeroed_ + 7) & ~uint64_t{7})));  // a prefix
    off_[n_] = (bytes_ + sizeof(T) - 1) / sizeof(T) * sizeof(T);
    ptr_[n_] = p;
    bytes_ = off_[n_++] + sizeof(T) * n;
    if (zeroed) zeroed_ = bytes_;
  }
  uint64_t bytes() const { return bytes_; }
  uint64_t zeroed() const { return std::min((zeroed_ + 7) & ~uint64_t{7}, bytes_); }  // whole 8-byte words
  void bind(void *base) const {
    for (uint32_t i = 0; i < n_; ++i) {
      char *const at = static_cast<char *>(base) + off_[i];
      std::memcpy(ptr_[i], &at, sizeof at);  // *ptr_[i] is a T *: every object pointer has this size
    }
  }

 private:
  static constexpr uint32_t kMaxArrays = 16;
  uint64_t off_[kMaxArrays], bytes_ = 0, zeroed_ = 0;
  void *ptr_[kMaxArrays];
  uint32_t n_ = 0;
};

// ---- the LDS plan ---------------------------------------------------------------------------

constexpr uint32_t kCus = 256;       // MI355X: the persistent grids of the group queries
constexpr uint32_t kMaxCopies = 64;  // one copy of a group query's LDS bins per lane of a wave

// The power-of-two copies of per_copy words (the caller's odd stride: the copies of a bin fall
// into different banks) that fit in `words`, at most kMaxCopies; 1 when not even one fits.
inline uint32_t copies_that_fit(uint32_t per_copy, uint32_t words) {
  uint32_t copies = 1;
  while (copies < kMaxCopies && 2 * copies * per_copy <= words) copies *= 2;
  return copies;
}

// Replicated bins in the small LDS size, one copy in the big one, more groups than LDS holds.
enum Regime { kSmall = 0, kBig = 1, kOver = 2 };
struct Lds {  // a unit's constants: its LDS sizes in words and its workgroups per CU by regime
  uint32_t small_words, big_words, pass_words, per_cu[3];  // pass_words 0: kOver has no passes
};
struct Bins {
  Regime regime;
  uint32_t copies;        // kSmall: 2^k copies
  uint32_t bins, passes;  // kOver with passes: groups per pass, passes > 1; else n_groups, 1
  uint32_t wgs;           // the persistent workgroups the regime's kernel can keep resident
};
// per_copy: the words of one copy of every group's bins at its odd stride(s); group_words: of one group.
inline Bins plan_bins(const Lds &u, uint32_t n_groups, uint32_t per_copy, uint32_t group_words) {
  Bins b{kBig, 1, n_groups, 1, 0};
  if (per_copy <= u.small_words) {
    b.regime = kSmall;
    b.copies = copies_that_fit(per_copy, u.small_words);
  } else if (n_groups * group_words > u.big_words) {
    b.regime = kOver;
    if (u.pass_words) b.bins = u.pass_words / group_words;
    b.passes = (n_groups + b.bins - 1) / b.bins;
  }
  b.wgs = kCus * u.per_cu[b.regime];
  return b;
}
// The workgroups that share a batch's tiles (a pass's: its pass_tiles).
inline uint32_t plan_splits(const Bins &b, uint32_t tiles, uint32_t pass_tiles) {
  return std::max(1u, b.passes > 1 ? std::min(pass_tiles, b.wgs / b.passes) : std::min(tiles, b.wgs));
}

// The units' constants and the words they plan with.
constexpr Lds kGroupLds{4096, 9984, 9728, {3, 2, 2}};    // kacc_group.hip, u64 words: 1 + 2Z a group
constexpr Lds kHistLds{8192, 20096, 19200, {3, 1, 2}};   // kacc_hist.hip, u32 words: n_bounds + 5 a group
constexpr Lds kWindowLds{4096, 9984, 0, {3, 2, 8}};      // kacc_window.hip's read, u64 words: 1 + Z a group
constexpr uint32_t kDigitWords = 16384, kDigits = 256;   // kacc_quant.hip, kacc_gtop.hip: u32 digit counters

inline Bins group_bins(uint32_t n_groups, uint32_t Z) {
  return plan_bins(kGroupLds, n_groups, (n_groups * (1u + 2u * Z)) | 1u, 1u + 2u * Z);
}
inline Bins hist_bins(uint32_t n_groups, uint32_t n_bounds) {  // the counters' and the u64 sums' odd strides
  const uint32_t C = n_bounds + 3u;
  return plan_bins(kHistLds, n_groups, ((n_groups * C) | 1u) + 2u * (n_groups | 1u), C + 2u);
}
inline Bins window_bins(uint32_t n_groups, uint32_t Z) {
  return plan_bins(kWindowLds, n_groups, (n_groups * (1u + Z)) | 1u, 1u + Z);
}
// The copies of `counters` * 256 digit counters in LDS (use_lds: they are not in global memory);
// more than one copy: at the odd stride.
inline uint32_t digit_copies(uint32_t counters, bool use_lds) {
  return use_lds ? copies_that_fit((counters * kDigits) | 1u, kDigitWords) : 1u;
}

}  // namespace plan
}  // namespace kacc
