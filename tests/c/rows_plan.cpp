// TEST INFRASTRUCTURE: the host arithmetic of the row queries (kepler_amd/csrc/kacc_plan.hpp) as a
// stand-alone program, built by the host compiler alone (tests/test_rows_plan.py, once more with
// the address and undefined-behaviour sanitizers).  One request per line of standard input, one
// answer per line of standard output:
//   group G Z TILES PASS_TILES | hist G BOUNDS TILES PASS_TILES | window G Z TILES
//       -> the same words, then: regime copies bins passes wgs splits
//   digit COUNTERS          (the queries of kacc_quant.hip, the groups of kacc_gtop.hip)
//       -> digit COUNTERS copies          (0: the counters are in global memory)
//   layout ELEM:COUNT:ZEROED ...           (a call's arrays in order; ELEM is 1, 2, 4, 8 or 16 bytes)
//       -> layout BYTES ZEROED OFFSET ...  and every array is written through its own pointer
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../kepler_amd/csrc/kacc_plan.hpp"

namespace plan = kacc::plan;

struct Wide {  // a 16-byte element, as the top lists' and the selection's vector types
  alignas(16) uint64_t w[2];
};

static void print_bins(const std::string &line, const plan::Bins &b, uint32_t tiles, uint32_t pass_tiles) {
  static const char *const kNames[] = {"small", "big", "over"};
  std::printf("%s %s %u %u %u %u %u\n", line.c_str(), kNames[b.regime], b.copies, b.bins, b.passes, b.wgs,
              plan::plan_splits(b, tiles, pass_tiles));
}

template <class T>
static void add_array(plan::Layout &l, std::vector<void *> &ptrs, uint64_t n, bool zeroed) {
  ptrs.push_back(nullptr);  // reserved by the caller: the element's address is stable
  l.add(reinterpret_cast<T **>(&ptrs.back()), n, zeroed);
}

static int layout(std::istringstream &in) {
  struct Decl {
    uint64_t elem, n;
    int zeroed;
  };
  std::vector<Decl> decls;
  std::string tok;
  while (in >> tok) {
    Decl d{};
    if (std::sscanf(tok.c_str(), "%" SCNu64 ":%" SCNu64 ":%d", &d.elem, &d.n, &d.zeroed) != 3) return 1;
    decls.push_back(d);
  }
  plan::Layout l;
  std::vector<void *> ptrs;
  ptrs.reserve(decls.size());
  for (const Decl &d : decls) {
    switch (d.elem) {
      case 1: add_array<uint8_t>(l, ptrs, d.n, d.zeroed); break;
      case 2: add_array<uint16_t>(l, ptrs, d.n, d.zeroed); break;
      case 4: add_array<uint32_t>(l, ptrs, d.n, d.zeroed); break;
      case 8: add_array<uint64_t>(l, ptrs, d.n, d.zeroed); break;
      case 16: add_array<Wide>(l, ptrs, d.n, d.zeroed); break;
      default: return 1;
    }
  }
  // an allocation of exactly bytes(): a write outside it is the address sanitizer's to report
  char *const at = static_cast<char *>(std::malloc(l.bytes() ? l.bytes() : 1));
  if (!at) return 1;
  l.bind(at);
  std::memset(at, 0, l.zeroed());
  std::printf("layout %" PRIu64 " %" PRIu64, l.bytes(), l.zeroed());
  for (size_t i = 0; i < decls.size(); ++i) {
    std::memset(ptrs[i], 0x5a, decls[i].elem * decls[i].n);
    std::printf(" %td", static_cast<char *>(ptrs[i]) - at);
  }
  std::printf("\n");
  std::free(at);
  return 0;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string what;
    uint32_t g = 0, p = 0, tiles = 0, pass_tiles = 0;
    if (!(in >> what)) continue;
    if (what == "layout") {
      if (layout(in)) return 1;
    } else if (what == "digit" && in >> g) {
      const bool lds = g <= plan::kDigitWords / plan::kDigits;
      std::printf("digit %u %u\n", g, lds ? plan::digit_copies(g, true) : 0u);
    } else if (what == "group" && in >> g >> p >> tiles >> pass_tiles) {
      print_bins(line, plan::group_bins(g, p), tiles, pass_tiles);
    } else if (what == "hist" && in >> g >> p >> tiles >> pass_tiles) {
      print_bins(line, plan::hist_bins(g, p), tiles, pass_tiles);
    } else if (what == "window" && in >> g >> p >> tiles) {
      print_bins(line, plan::window_bins(g, p), tiles, 0u);
    } else {
      std::fprintf(stderr, "bad request: %s\n", line.c_str());
      return 1;
    }
  }
  return 0;
}
