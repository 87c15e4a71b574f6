// sf_zpaq_step.hpp -- the per-byte step of the reference's content-defined
// chunker (cdchunking's ZPAQ, src/index.rs:622-625), shared by the host cutter
// (sf_zpaq.cpp) and the device cutter (sf_cdc.hip) so the two cannot drift.
// constexpr functions: the host compiler and the device compiler both take
// them as they are.
//
// State of a chunk in progress: h (32-bit rolling hash), c1 (the previous
// byte, 0 at a chunk's first byte), o1[256] (order-1 table: the byte that last
// followed each byte, all 0 at a chunk's first byte) and the chunk's length
// so far.  For input byte b:
//     h  = h * (b == o1[c1] ? HM : 2 * HM) + b + 1   (mod 2^32)
//     o1[c1] = b;  c1 = b
// and the chunk ends AFTER b when h < 2^(32 - bits) or its length reaches
// max_size.  A fresh state has h = HM (not 0: with 0 the first byte always
// cuts), and the state is fresh again after every cut (the one
// assumption the reference's known-answer test does not pin).
#pragma once
#include <stdint.h>

namespace sfz {

constexpr uint32_t kHM = 123456791u;
constexpr uint32_t kFreshH = kHM;

// 1 <= bits <= 31
constexpr uint32_t limit(uint32_t bits) { return 1u << (32u - bits); }

// h after byte b, `predicted` = o1[c1] before this byte's table update
constexpr uint32_t step(uint32_t h, uint32_t b, uint32_t predicted) {
  return h * (b == predicted ? kHM : 2u * kHM) + b + 1u;
}

// does the chunk end after the byte that gave h?  run = its length with that byte
constexpr bool cuts(uint32_t h, uint32_t lim, uint32_t run, uint32_t max_size) {
  return h < lim || run == max_size;
}

}  // namespace sfz
