// sf_plan_copies.hpp -- the per-block rules of sf_plan_copies.hip (include/
// syncfast_amd.h: sf_plan_copies_device): what becomes of a received
// FILE_BLOCK whose hash the destination's table may hold (classify), which
// inputs are refused (row_ok, file_ok, section_ok, dst_of, in_arena) and the
// digest comparison that turns a candidate into a job (same_digest).  The
// reference copies every block get_block finds (src/sync/fs.rs:461-471); here
// a row of another size, a file shorter than its row says, a file that is not
// loaded and bytes that no longer hash to the announced digest are left for
// the source to send.
//
// No HIP and no library header (tests/native/plan_copies.cpp executes them on
// a CPU), and every function is constexpr: the kernels call the same ones, so
// host and device cannot disagree about a class.
#pragma once
#include <stdint.h>

namespace sfpc {

constexpr uint32_t kDigest = 20;
constexpr uint64_t kNotLoaded = UINT64_MAX;  // d_local_base[j] of a file the caller did not load

// The classes, in the order they are tried; a block gets the first that
// applies.  kJob and kUnverified are what verification makes of a candidate;
// kNone is a lane without a block.
enum Class : uint8_t {
  kMissing = 0, kSizeMismatch = 1, kStale = 2, kUnavailable = 3, kEmpty = 4, kCandidate = 5,
  kJob = 6, kUnverified = 7, kNone = 8
};

// Bad input (SF_ERANGE): a found row outside the table, a row of a local file
// outside the local lists, a block of a section outside the bases.
constexpr bool row_ok(int64_t r, uint64_t n_table) { return r < 0 || (uint64_t)r < n_table; }
constexpr bool file_ok(uint32_t j, uint64_t n_local) { return j < n_local; }
constexpr bool section_ok(uint32_t f, uint64_t n_files) { return f < n_files; }

// *dst = base + offset, where the block lies in the image allocation; false
// when the sum passes 2^64 - 1.
constexpr bool dst_of(uint64_t base, uint64_t offset, uint64_t* dst) {
  if (offset > UINT64_MAX - base) return false;
  *dst = base + offset;
  return true;
}

// A candidate's bytes [base + offset, + size) lie in the arena's [0, src_len).
constexpr bool in_arena(uint64_t base, uint64_t offset, uint32_t size, uint64_t src_len) {
  if (offset > UINT64_MAX - base) return false;
  const uint64_t at = base + offset;
  return at <= src_len && size <= src_len - at;
}

// The class of a block of `size` bytes found in a row (r >= 0, row_ok and
// file_ok) of t_size bytes at t_offset of a local file of l_size bytes that
// lies at l_base of the arena (a query has no bases: pass 0).
constexpr Class classify(int64_t r, uint32_t size, uint32_t t_size, uint64_t t_offset, uint64_t l_size,
                         uint64_t l_base) {
  if (r < 0) return kMissing;
  if (t_size != size) return kSizeMismatch;
  if (t_offset > l_size || size > l_size - t_offset) return kStale;
  if (l_base == kNotLoaded) return kUnavailable;
  if (size == 0) return kEmpty;
  return kCandidate;
}

// The row's present flag: the block needs nothing from the source.
constexpr bool present(uint8_t cls, uint8_t job_class) { return cls == job_class || cls == kEmpty; }

// Two digests as five 32-bit words each (both tables are 4-B aligned).
constexpr bool same_digest(const uint32_t* a, const uint32_t* b) {
  uint32_t d = 0;
  for (uint32_t w = 0; w < kDigest / 4; w++) d |= a[w] ^ b[w];
  return d == 0;
}

}  // namespace sfpc
