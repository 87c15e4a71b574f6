// sf_want_plan.hpp -- the per-row rules of sf_want.hip (include/
// syncfast_amd.h: sf_wire_get_blocks_device, sf_place_block_data_device):
// which rows of a destination's table ask for their block (asks), the GET_BLOCK
// message a row becomes (write_get_block, written by src/sync/ssh/proto.rs:
// 170-174) and what a row does with the message the lookup found for it
// (place).
//
// No HIP and no library header (tests/native/want_plan.cpp executes them on a
// CPU), and every function is constexpr: the kernels call the same ones, so
// host and device cannot disagree about a flag or a byte.
#pragma once
#include "sf_wire_data.hpp"

namespace sfwt {

// Row i asks when the receive's lookup found no block for it (rows NULL: no
// such array) and the caller's flag takes it (take NULL: all).
constexpr bool asks(const int64_t* rows, const uint8_t* take, uint64_t i) {
  return (!rows || rows[i] < 0) && (!take || take[i] != 0);
}

// "GET_BLOCK\n" + digest[0, 20) + "\n" at out[0, 31): byte stores only, none
// outside.  The digest's bytes are taken as they are.
constexpr void write_get_block(uint8_t* out, const uint8_t* digest) {
  const char tag[sfwp::kGetTag] = {'G', 'E', 'T', '_', 'B', 'L', 'O', 'C', 'K', '\n'};
  for (uint32_t k = 0; k < sfwp::kGetTag; k++) out[k] = (uint8_t)tag[k];
  for (uint32_t k = 0; k < sfwp::kDigest; k++) out[sfwp::kGetTag + k] = digest[k];
  out[sfwp::kGetTag + sfwp::kDigest] = '\n';
}

// What becomes of a row: nothing (it is present already, or no ok message
// carries its digest), a job (the message's payload has the row's size), or a
// size mismatch (it has another: the row stays missing).
enum Place { kNone = 0, kJob = 1, kMismatch = 2 };
constexpr Place place(uint8_t present, int64_t msg, uint32_t msg_size, uint32_t row_size) {
  if (present != 0 || msg < 0) return kNone;
  return msg_size == row_size ? kJob : kMismatch;
}

}  // namespace sfwt
