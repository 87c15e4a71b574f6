// layout.cpp -- the scratch layout and the launch pieces of the device entry
// points (syncfast_amd/csrc/sf_layout.hpp) executed on a CPU: a stand-alone
// program, built with ASan + UBSan by tests/test_layout.py and run directly.
//
// A layout's parts are taken from a heap block of exactly total() bytes and
// every part is filled over its whole declared size, so a part that leaves the
// allocation or runs into its neighbour is caught twice -- by the check here
// and by the sanitizer.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <utility>
#include <vector>

#include "../../syncfast_amd/csrc/sf_layout.hpp"

using sfi::ScratchLayout;

#define REQUIRE(c)                                                 \
  do {                                                             \
    if (!(c)) {                                                    \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
      exit(1);                                                     \
    }                                                              \
  } while (0)

static uint64_t g_cases = 0;

// The parts `sizes` in declaration order: offsets on 256-byte boundaries, in
// order, no part inside another, total() = the last offset + its rounded size.
static void check_layout(const std::vector<size_t>& sizes) {
  ScratchLayout L;
  REQUIRE(L.total() == 0);
  std::vector<size_t> at;
  size_t end = 0;  // where the parts so far end, rounded
  for (size_t b : sizes) {
    const size_t o = L.add(b);
    REQUIRE(o % 256 == 0);
    REQUIRE(o == end);  // declaration order, nothing between two parts but the rounding
    end = o + (b + 255) / 256 * 256;
    REQUIRE(end >= o + b && end - (o + b) < 256);
    REQUIRE(L.total() == end);
    at.push_back(o);
  }
  // one allocation of exactly total() bytes; part k filled with k + 1
  uint8_t* base = static_cast<uint8_t*>(malloc(L.total() ? L.total() : 1));
  REQUIRE(base);
  memset(base, 0, L.total());
  for (size_t k = 0; k < sizes.size(); k++) {
    uint8_t* p = ScratchLayout::at<uint8_t>(base, at[k]);
    REQUIRE(p == base + at[k]);
    for (size_t j = 0; j < sizes[k]; j++) {
      REQUIRE(p[j] == 0);  // no earlier part reaches into this one
      p[j] = (uint8_t)(k + 1);
    }
  }
  for (size_t k = 0; k < sizes.size(); k++)
    for (size_t j = 0; j < sizes[k]; j++) REQUIRE(base[at[k] + j] == (uint8_t)(k + 1));
  // a typed pointer is the same address
  if (!sizes.empty()) REQUIRE(reinterpret_cast<uint8_t*>(ScratchLayout::at<uint64_t>(base, at.back())) == base + at.back());
  free(base);
  g_cases++;
}

static void layouts() {
  check_layout({});
  check_layout({0});
  check_layout({1});
  check_layout({255, 256, 257});
  check_layout({8, 0, 8});        // a zero-byte part shares its offset with the next
  check_layout({16, 20 * 7, 8 * 7, 8 * 7, 4 * 7});  // sf_send.hip's request scratch for 7 slots
  // the conditional part of sf_want.hip: n * 8, (distinct ? n * 8 : 0), n
  for (size_t n : {1, 31, 32, 33, 1000}) {
    for (int distinct = 0; distinct < 2; distinct++) {
      ScratchLayout L;
      const size_t ends = L.add(n * 8), found = L.add(distinct ? n * 8 : 0), ask = L.add(n);
      const size_t eb = sfi::align256(n * 8), fb = sfi::align256(n);
      REQUIRE(ends == 0 && found == eb && ask == eb + (distinct ? eb : 0));
      REQUIRE(L.total() == eb + (distinct ? eb : 0) + fb);
      check_layout({n * 8, distinct ? n * 8 : (size_t)0, n});
    }
  }
  // sizes around every boundary up to a few parts
  for (size_t a = 0; a <= 513; a += (a % 256 == 1 ? 254 : 1))
    for (size_t b : {0, 1, 256, 300}) check_layout({a, b, a});
}

static void pieces() {
  const uint64_t max = 4;
  for (uint64_t n : {0, 1, 3, 4, 5, 13}) {
    std::vector<std::pair<uint64_t, uint64_t>> got;
    const int rc = sfi::for_pieces(n, max, [&](uint64_t first, uint64_t count) {
      got.push_back({first, count});
      return 0;
    });
    REQUIRE(rc == 0);
    REQUIRE(got.size() == (n + max - 1) / max);  // no call for n = 0, no empty piece
    uint64_t next = 0;
    for (const auto& p : got) {  // in order, tiling [0, n) exactly
      REQUIRE(p.first == next);
      REQUIRE(p.second >= 1 && p.second <= max);
      next += p.second;
    }
    REQUIRE(next == n);
    for (size_t k = 0; k + 1 < got.size(); k++) REQUIRE(got[k].second == max);  // only the last is short
    g_cases++;
    // an error from the k-th call ends the loop and is what comes back
    for (uint64_t fail = 0; fail < got.size(); fail++) {
      uint64_t calls = 0;
      const int erc = sfi::for_pieces(n, max, [&](uint64_t first, uint64_t count) {
        REQUIRE(first == got[calls].first && count == got[calls].second);
        return calls++ == fail ? -7 - (int)fail : 0;
      });
      REQUIRE(erc == -7 - (int)fail);
      REQUIRE(calls == fail + 1);
      g_cases++;
    }
  }
  // the bound the entry points pass: nothing is split at or below it
  uint64_t calls = 0;
  REQUIRE(sfi::for_pieces(1ull << 30, 1ull << 30, [&](uint64_t first, uint64_t count) {
            calls++;
            return first == 0 && count == 1ull << 30 ? 0 : -1;
          }) == 0 && calls == 1);
  calls = 0;
  REQUIRE(sfi::for_pieces((1ull << 30) + 1, 1ull << 30, [&](uint64_t first, uint64_t count) {
            calls++;
            return (first == 0 && count == 1ull << 30) || (first == 1ull << 30 && count == 1) ? 0 : -1;
          }) == 0 && calls == 2);
  g_cases += 2;
}

int main() {
  layouts();
  pieces();
  printf("ok %llu\n", (unsigned long long)g_cases);
  return 0;
}
