// copy_plan.cpp -- the plan of the block copy kernel (syncfast_amd/csrc/
// sf_copy_plan.hpp) executed on a CPU, piece by piece as the kernel executes
// it: a stand-alone program, built with ASan + UBSan by tests/test_copy_plan.py
// and run directly.
//
// Addresses are modelled: the source buffer lies at virtual addresses
// [lo, hi) and is a heap copy of exactly hi - lo bytes, the job's destination
// range [D, D + n) a heap copy of exactly n bytes, so a modelled load or store
// outside them is caught twice -- by the check here and by the sanitizer.
// For every job the stores must cover the destination bytes exactly once and
// nothing else, the loads must stay inside the source buffer, and the bytes
// that arrive must be the source's.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../syncfast_amd/csrc/sf_copy_plan.hpp"

using namespace sfcp;

static uint64_t g_fast = 0, g_bytewise = 0, g_jobs = 0;

#define REQUIRE(c)                                                 \
  do {                                                             \
    if (!(c)) {                                                    \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
      exit(1);                                                     \
    }                                                              \
  } while (0)

struct Source {
  uint64_t lo, hi;  // virtual addresses
  uint8_t* heap;    // hi - lo bytes
  void load(uint64_t at, uint64_t bytes, void* out) const {
    REQUIRE(at >= lo && at + bytes <= hi && at + bytes >= at);
    memcpy(out, heap + (at - lo), bytes);
  }
};

struct Dest {
  uint64_t D, n;
  uint8_t* heap;  // n bytes
  uint8_t* hits;  // n counters
  void store(uint64_t at, uint64_t bytes, const void* in) {
    REQUIRE(at >= D && at + bytes <= D + n);
    memcpy(heap + (at - D), in, bytes);
    for (uint64_t i = 0; i < bytes; i++) hits[at - D + i]++;
  }
};

// One job, as copy_tiles_kernel runs it: S, D the addresses of its first
// source and destination byte; the source buffer has `lead` bytes before the
// job's range and `trail` after it.
static void run_job(uint64_t S, uint64_t D, uint32_t n, uint32_t lead, uint32_t trail) {
  g_jobs++;
  const uint64_t len = (uint64_t)lead + n + trail;
  std::vector<uint8_t> pattern(len);
  for (uint64_t i = 0; i < len; i++) pattern[i] = (uint8_t)(i * 131 + (i >> 8) * 7 + S + 3 * D + 1);
  Source src{S - lead, S + n + trail, (uint8_t*)malloc(len ? len : 1)};
  if (len) memcpy(src.heap, pattern.data(), len);
  Dest dst{D, n, (uint8_t*)malloc(n ? n : 1), (uint8_t*)calloc(n ? n : 1, 1)};
  const uint64_t delta = S - D;

  const uint64_t tiles = tile_count(D, n);
  REQUIRE((n == 0) == (tiles == 0));
  uint64_t at = D;
  for (uint64_t k = 0; k < tiles; k++) {
    const Tile t = tile_range(D, n, k);
    REQUIRE(t.a == at && t.a < t.e && t.e <= D + n);             // tiles follow each other, none is empty
    REQUIRE((t.a >> kTileBits) == ((t.e - 1) >> kTileBits));     // one window of the destination
    REQUIRE(k == 0 || (t.a & (kTile - 1)) == 0);                 // inner edges are T-aligned
    at = t.e;
    const Split sp = split(t.a, t.e);
    REQUIRE(t.a <= sp.h && sp.h <= sp.b && sp.b <= t.e);
    REQUIRE(sp.h - t.a < kVec && t.e - sp.b < kVec);             // at most 15 byte stores at each end
    REQUIRE((sp.b - sp.h) % kVec == 0 && (sp.b == sp.h || sp.h % kVec == 0));
    REQUIRE((sp.b - sp.h) / kVec <= kTileChunks);
    REQUIRE(k == 0 || sp.h == t.a);                              // only the first tile has a head
    REQUIRE(k == tiles - 1 || sp.b == t.e);                      // only the last a tail
    for (uint64_t q = t.a; q < sp.h; q++) {
      uint8_t b;
      src.load(q + delta, 1, &b);
      dst.store(q, 1, &b);
    }
    for (uint64_t q = sp.h; q < sp.b; q += kVec) {
      const uint64_t s = q + delta;
      const Load L = chunk_load(s, src.lo, src.hi);
      uint32_t w[4];
      if (L.dwords) {
        REQUIRE(L.at % 4 == 0 && L.at <= s && L.shift == s - L.at && L.dwords == (L.shift ? 5u : 4u));
        uint32_t d[5] = {0, 0, 0, 0, 0};
        src.load(L.at, 4ull * L.dwords, d);
        for (int j = 0; j < 4; j++) w[j] = shifted(d[j], d[j + 1], L.shift);
        g_fast++;
      } else {
        REQUIRE(L.at == s);
        uint8_t b[16];
        for (int j = 0; j < 16; j++) src.load(s + j, 1, &b[j]);
        memcpy(w, b, 16);
        g_bytewise++;
      }
      dst.store(q, kVec, w);
    }
    for (uint64_t q = sp.b; q < t.e; q++) {
      uint8_t b;
      src.load(q + delta, 1, &b);
      dst.store(q, 1, &b);
    }
  }
  REQUIRE(at == D + n || n == 0);
  for (uint32_t i = 0; i < n; i++) {
    REQUIRE(dst.hits[i] == 1);
    REQUIRE(dst.heap[i] == pattern[lead + i]);
  }
  free(src.heap);
  free(dst.heap);
  free(dst.hits);
}

static void range_rules() {
  const uint64_t top = ~0ull;
  REQUIRE(in_range(0, 0, 0) && in_range(0, 10, 10) && in_range(10, 0, 10) && in_range(3, 7, 10));
  REQUIRE(!in_range(0, 11, 10) && !in_range(10, 1, 10) && !in_range(11, 0, 10) && !in_range(4, 7, 10));
  REQUIRE(!in_range(top, 2, 10) && !in_range(top, 2, top) && !in_range(top, 0, 10) && !in_range(top - 1, 2, top - 1));
  REQUIRE(in_range(top, 0, top) && in_range(top - 2, 2, top) && !in_range(top - 1, 2, top));
  REQUIRE(in_range(0, 0xFFFFFFFFu, 1ull << 32) && !in_range(2, 0xFFFFFFFFu, 1ull << 32));
  REQUIRE(tile_count(0, 0) == 0 && tile_count(12345, 0) == 0);
  REQUIRE(tile_count(0, 1) == 1 && tile_count(kTile - 1, 1) == 1 && tile_count(kTile - 1, 2) == 2);
  REQUIRE(tile_count(0, (uint32_t)kTile) == 1 && tile_count(1, (uint32_t)kTile) == 2);
  REQUIRE(tile_count(5, 0xFFFFFFFFu) == (1ull << (32 - kTileBits)) + 1);
  REQUIRE(tile_count(0, 0xFFFFFFFFu) == 1ull << (32 - kTileBits));
  REQUIRE((kTile & (kTile - 1)) == 0 && kTile >= 64 * kVec);
}

int main() {
  range_rules();
  std::vector<uint32_t> sizes;
  for (uint32_t n = 0; n <= 80; n++) sizes.push_back(n);
  for (uint32_t n : {(uint32_t)kTile - 1, (uint32_t)kTile, (uint32_t)kTile + 1, 2 * (uint32_t)kTile + 1}) sizes.push_back(n);
  // the destination starts in a window's first 16 bytes, and 40 bytes before
  // a window's end (small jobs cross into the next tile)
  const uint64_t dst_bases[2] = {0x40000, 0x40000 + kTile - 40};
  // the source buffer: exactly the job's range; ending exactly at its end;
  // starting exactly at its start; room on both sides
  const uint32_t room[4][2] = {{0, 0}, {24, 0}, {0, 24}, {24, 24}};
  for (uint32_t sa = 0; sa < 16; sa++)
    for (uint32_t da = 0; da < 16; da++)
      for (uint32_t n : sizes)
        for (uint64_t base : dst_bases)
          for (const auto& r : room) run_job(0x9000000 + sa, base + da, n, r[0], r[1]);
  // a source below its destination and far above it (S - D wraps either way)
  run_job(0x1003, 0x7000005, 3 * (uint32_t)kTile + 7, 0, 0);
  run_job(0x7000005ull << 8, 0x1003, 3 * (uint32_t)kTile + 7, 0, 0);
  REQUIRE(g_fast > 100000 && g_bytewise > 10000);  // both kinds of load were exercised
  printf("ok %llu jobs, %llu dword chunks, %llu bytewise chunks\n", (unsigned long long)g_jobs,
         (unsigned long long)g_fast, (unsigned long long)g_bytewise);
  return 0;
}
