// sf_cdc_lane.hpp -- one lane of the device ZPAQ cutters: the chunker whose
// order-1 table lives in LDS (LaneChunker) and the writer of a segment's cut
// bitmap words (CutWriter).  Device code, included by the cutters' translation
// units only (sf_cdc.hip: one buffer; sf_cdc_files.hip: many files), inside
// their anonymous namespaces' reach: everything here is inlined into their
// kernels.  The LDS layout is described in sf_cdc.hip's file comment.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sf_zpaq_step.hpp"

namespace {

constexpr uint32_t kLanes = 64;           // one wave per workgroup

// One lane's chunker: the order-1 table lives in LDS at tab[...] (see the
// file comment for the layout; tab already points at this lane's column).
struct LaneChunker {
  uint8_t* tab;
  uint32_t lim, max_size, h, c1, run;
  __device__ __forceinline__ void fresh() {
    h = sfz::kFreshH;
    c1 = 0;
    run = 0;
    uint32_t* t = reinterpret_cast<uint32_t*>(tab);
#pragma unroll 8
    for (uint32_t k = 0; k < 64; k++) t[k * kLanes] = 0;
  }
  __device__ __forceinline__ uint8_t* entry(uint32_t c) const { return tab + ((c >> 2) << 8) + (c & 3); }
  // feeds one byte; true: the chunk ends after it (the state is fresh again)
  __device__ __forceinline__ bool feed(uint32_t b) {
    uint8_t* e = entry(c1);
    h = sfz::step(h, b, *e);
    *e = (uint8_t)b;
    c1 = b;
    run++;
    if (!sfz::cuts(h, lim, run, max_size)) return false;
    fresh();
    return true;
  }
  // Feeds 16 bytes with no branch per byte: the table's reads and writes
  // depend on the data only, not on h, so they form one in-order LDS stream
  // whose latency overlaps the multiply chain.  Returns the index of the
  // first byte that ends a chunk (the state is then fresh: the table writes
  // made for the bytes after it are wiped with the rest), or 16.
  __device__ __forceinline__ uint32_t feed16(const uint4& v) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t pr[16], c = c1;
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) {
      const uint32_t b = (w[k >> 2] >> (8 * (k & 3))) & 0xFFu;
      uint8_t* e = entry(c);
      pr[k] = *e;
      *e = (uint8_t)b;
      c = b;
    }
    uint32_t hh = h, first = 16;
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) {
      hh = sfz::step(hh, (w[k >> 2] >> (8 * (k & 3))) & 0xFFu, pr[k]);
      const bool ct = sfz::cuts(hh, lim, run + k + 1, max_size);
      first = ct && first == 16 ? k : first;
    }
    if (first == 16) {
      h = hh;
      c1 = c;
      run += 16;
    } else {
      fresh();
    }
    return first;
  }
  // The 64 bytes fetched ahead: rk = the 16 bytes at rpos + 16 k, loaded
  // while they lie below hi.
  uint4 r0, r1, r2, r3;
  uint64_t rpos;
  // Feeds ONE unit of bytes [p, hi) (hi <= the buffer's length; the same hi
  // in every call of a run): 16 bytes where the address is 16-byte aligned
  // and they are all in range, else 1.  Returns the position after the unit
  // and cut = false, or the position after the byte that ends a chunk and
  // cut = true.  One unit per call keeps the caller's loop flat: lanes on the
  // two paths, or just past a cut, cost each other one iteration, not a run.
  __device__ __forceinline__ uint64_t advance(const uint8_t* __restrict__ data, uint64_t p, uint64_t hi, bool& cut) {
    if (((reinterpret_cast<uintptr_t>(data + p) & 15) == 0) && hi - p >= 16) {
      const uint4* q = reinterpret_cast<const uint4*>(data + p);
      if (rpos != p) {
        r0 = q[0];
        if (hi - p >= 32) r1 = q[1];
        if (hi - p >= 48) r2 = q[2];
        if (hi - p >= 64) r3 = q[3];
      }
      const uint4 v = r0;
      r0 = r1;
      r1 = r2;
      r2 = r3;
      if (hi - p >= 80) r3 = q[4];
      rpos = p + 16;
      const uint32_t j = feed16(v);
      cut = j < 16;
      return cut ? p + j + 1 : p + 16;
    }
    cut = feed((uint32_t)data[p]);
    return p + 1;
  }
};

// Bit i of a cut bitmap = a chunk ends after byte i.  Segment s owns words
// [s * L / 32, ceil(min(len, (s + 1) * L) / 32)).  A segment's cuts arrive in
// increasing order; the words between them are zero.
struct CutWriter {
  uint32_t* a;
  uint32_t* b;  // a second bitmap that gets the same words, or NULL
  uint64_t w;   // the word being gathered
  uint32_t acc;
  __device__ __forceinline__ void store(uint64_t k, uint32_t v) {
    a[k] = v;
    if (b) b[k] = v;
  }
  __device__ __forceinline__ void advance(uint64_t wi) {  // w < wi: words [w, wi) are complete
    store(w, acc);
    for (uint64_t k = w + 1; k < wi; k++) store(k, 0u);
    w = wi;
    acc = 0;
  }
  __device__ __forceinline__ void put(uint64_t i) {  // a chunk ends after byte i
    if ((i >> 5) != w) advance(i >> 5);
    acc |= 1u << (i & 31);
  }
  __device__ __forceinline__ void finish(uint64_t wend) { advance(wend + 1); }  // through word wend
};

}  // namespace
