// sf_copy_plan.hpp -- the arithmetic of the block copy kernel (sf_copy.hip,
// include/syncfast_amd.h: sf_copy_blocks_device): which jobs are copied at
// all (in_range), how a job is cut into tiles (tile_count, tile_range), how a
// tile's bytes are stored (split: byte stores at the edges, aligned 16-byte
// stores between) and where the bytes of one 16-byte store are loaded from
// (chunk_load: aligned dwords shifted into place, or byte by byte where a
// dword would leave the source buffer).
//
// Everything here works on addresses as integers.  No HIP and no library
// header (tests/native/copy_plan.cpp executes the plan on a CPU), and every
// function is constexpr: the kernel calls the same ones, so what the host
// test proves about stores and loads holds for the kernel's.
#pragma once
#include <stdint.h>

namespace sfcp {

constexpr uint32_t kTileBits = 12;
constexpr uint64_t kTile = 1ull << kTileBits;  // T: bytes of a tile, on T-aligned destination addresses
constexpr uint64_t kVec = 16;                  // bytes of a body store
constexpr uint32_t kTileChunks = (uint32_t)(kTile / kVec);  // body stores of a whole tile

// [off, off + size) lies in [0, len): also when off + size passes 2^64.
constexpr bool in_range(uint64_t off, uint32_t size, uint64_t len) { return off <= len && size <= len - off; }

// Tiles of the job that writes `size` bytes at destination address D: the
// T-aligned windows of the address space its bytes fall into.
constexpr uint64_t tile_count(uint64_t D, uint32_t size) {
  return size ? ((D + size - 1) >> kTileBits) - (D >> kTileBits) + 1 : 0;
}

// Destination addresses [a, e) of tile k (< tile_count) of that job: the
// job's bytes in window (D / T) + k.  Never empty.
struct Tile {
  uint64_t a, e;
};
constexpr Tile tile_range(uint64_t D, uint32_t size, uint64_t k) {
  const uint64_t w = ((D >> kTileBits) + k) << kTileBits, end = D + size;
  return Tile{w > D ? w : D, w + kTile < end ? w + kTile : end};
}

// How [a, e) is stored: bytes [a, h) one by one (fewer than 16: up to the
// first 16-byte boundary, or to e), [h, b) in 16-byte stores on 16-byte
// boundaries, bytes [b, e) one by one (fewer than 16).  Only a job's first
// tile has a head and only its last a tail: inner tile edges are T-aligned.
struct Split {
  uint64_t h, b;
};
constexpr Split split(uint64_t a, uint64_t e) {
  const uint64_t up = (a + kVec - 1) & ~(kVec - 1);
  const uint64_t h = up < e ? up : e;
  return Split{h, h + ((e - h) & ~(kVec - 1))};
}

// The loads for the 16 source bytes at address s (any alignment) of a source
// buffer at addresses [lo, hi), s + 16 <= hi: `dwords` (4, or 5 when s is no
// multiple of 4) aligned dwords from address `at` <= s, of which the 16 bytes
// from byte `shift` on are the ones; dwords == 0 where those dwords would
// leave [lo, hi): then the 16 bytes are loaded one by one from s itself.
struct Load {
  uint64_t at;
  uint32_t dwords, shift;
};
constexpr Load chunk_load(uint64_t s, uint64_t lo, uint64_t hi) {
  const uint32_t shift = (uint32_t)(s & 3u), dwords = shift ? 5u : 4u;
  const uint64_t at = s - shift;
  return at >= lo && at + 4ull * dwords <= hi ? Load{at, dwords, shift} : Load{s, 0u, 0u};
}

// Dword j (0..3) of the 16 bytes, from the loaded dwords d[j] and d[j + 1]
// (little-endian; d[4] is not read when shift == 0).
constexpr uint32_t shifted(uint32_t d_lo, uint32_t d_hi, uint32_t shift) {
  return shift ? (d_lo >> (8 * shift)) | (d_hi << (32 - 8 * shift)) : d_lo;
}

}  // namespace sfcp
