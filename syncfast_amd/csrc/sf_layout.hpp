// sf_layout.hpp -- how a device entry point divides its one stream-ordered
// allocation, and how a launch over more items than one grid takes is cut into
// pieces.  Host arithmetic only (no HIP include): tests/native/layout.cpp
// executes it under ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace sfi {

// The parts of one allocation start on 256-byte boundaries.
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// Declare the parts, allocate total() bytes once, take the pointers:
//   ScratchLayout L;
//   const size_t ends = L.add(n * 8), flags = L.add(n);
//   stream_alloc(&p, L.total() + tail_bytes, s);
//   uint64_t* d_ends = L.at<uint64_t>(p, ends);
// A part of 0 bytes takes no room (it shares its offset with the next one).
// total() is itself a part's offset: a tail that needs no rounding -- the
// scan's temporary, which every entry point keeps last -- starts there.
class ScratchLayout {
 public:
  size_t add(size_t bytes) {
    const size_t at = total_;
    total_ += align256(bytes);
    return at;
  }
  size_t total() const { return total_; }
  template <typename T>
  static T* at(void* base, size_t offset) {
    return reinterpret_cast<T*>(static_cast<unsigned char*>(base) + offset);
  }

 private:
  size_t total_ = 0;
};

// fn(first, count) over [0, n) in consecutive pieces of at most `max` items,
// in order; the first result that is not 0 (SF_OK) ends the loop and is
// returned.  No call for n = 0.
template <typename F>
inline int for_pieces(uint64_t n, uint64_t max, F&& fn) {
  for (uint64_t first = 0; first < n; first += max) {
    const int rc = fn(first, n - first < max ? n - first : max);
    if (rc != 0) return rc;
  }
  return 0;
}

}  // namespace sfi
