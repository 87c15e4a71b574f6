// sf_recv_scan.hpp -- what the three receive parsers share (sf_recv.hip for
// FILE_BLOCK runs, sf_recv_data.hip for BLOCK_DATA runs, sf_recv_files.hip
// for a whole GetFiles stream; each stays its own translation unit with its
// own code objects): the first two steps of a parse, the bitmap reads of the
// chain kernels, the 32-to-64-bit widening of the size scans, and the upload
// of a run that lies in host memory.
//
// A message start cannot be told from digest or payload bytes that happen to
// hold the same bytes, so every parser first finds every position where a
// message could start and then decide, each in its own way, which of them
// chain from byte 0:
//
//   candidates  every byte position p is tested (a lane takes 16 of them): p
//               is a candidate when a whole, valid message stands there
//               (Rules::message: the function the host parser uses, so host
//               and device cannot disagree).  Every true message start is
//               one; a digest or a payload may forge others.  64 positions'
//               flags are one word of a bitmap and one count.
//   scan        rocprim inclusive scan of the counts: the candidates up to
//               and with each word, i.e. every candidate's index in position
//               order.
//
// What is particular to a message kind is a small stateless struct Rules:
//   static constexpr uint32_t kFirst, kSecond
//       the prefilter: only a position that holds the byte kFirst, followed
//       by kSecond unless that is 0, is looked at further (the tag's first
//       bytes, as far as they are rare enough in what a run carries);
//   static message(const uint8_t* b, uint64_t avail, uint32_t* H, uint64_t* size)
//       the test: the length of the whole valid message that stands at b, 0
//       when none does, reading no byte at or past b + avail -- block_message
//       or data_message as it is; H and size are theirs to write, the kernel
//       does not read them.
// (The prefilter is two constants and not a function of the lane's words,
// and the test's outputs are the kernel's, because with either as a function
// of its own the compiler orders a few operands and registers of the
// BLOCK_DATA kernel differently; as they stand both kernels compile to the
// instructions they had as two copies.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "sf_device.hpp"
#include "sf_stage.hpp"

namespace sfrs {

constexpr uint64_t kMaxRun = 1ull << 38;  // bytes per call: every grid stays far below 2^31 workgroups
constexpr uint32_t kPerLane = 16;         // byte positions per lane of the candidates kernel
constexpr uint64_t kUploadPiece = 64ull << 20;  // bytes of the run per pinned stage

// 0x80 in exactly the bytes of v that equal c
__device__ __forceinline__ uint32_t bytes_equal(uint32_t v, uint32_t c) {
  const uint32_t x = v ^ (c * 0x01010101u);
  return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}

// bytes_equal over a lane's 16 bytes: positions 0..7 in lo, 8..15 in hi
__device__ __forceinline__ void bytes_equal16(const uint32_t w[4], uint32_t c, unsigned long long& lo,
                                              unsigned long long& hi) {
  lo = bytes_equal(w[0], c) | (unsigned long long)bytes_equal(w[1], c) << 32;
  hi = bytes_equal(w[2], c) | (unsigned long long)bytes_equal(w[3], c) << 32;
}

// One lane per 16 byte positions [p0, p0 + 16): their bytes come as aligned
// dwords (data itself needs no alignment: the five dwords that hold them are
// shifted into place) where all five lie inside [data, data + n), else byte by
// byte, so nothing outside the run is read.  Only the positions the prefilter
// leaves are looked at further, one after the other: most lanes have one or
// none, so the wave tests one position at a time.  Four lanes' flags make one
// word of the bitmap.
template <class Rules>
__global__ void __launch_bounds__(256) candidates_kernel(const uint8_t* __restrict__ data, uint64_t n,
                                                         unsigned long long* __restrict__ words,
                                                         uint32_t* __restrict__ counts) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t p0 = g * kPerLane;
  uint32_t w[4] = {0, 0, 0, 0}, mask = 0;
  if (p0 < n) {
    const uint32_t a = (uint32_t)(reinterpret_cast<uintptr_t>(data) & 3u);  // the same for every lane: p0 is a multiple of 16
    if (p0 >= a && p0 - a + kPerLane + 4 <= n) {
      const uint32_t* q = reinterpret_cast<const uint32_t*>(data + p0 - a);
      const uint32_t d[5] = {q[0], q[1], q[2], q[3], a ? q[4] : 0u};
#pragma unroll
      for (int j = 0; j < 4; j++) w[j] = __funnelshift_r(d[j], d[j + 1], 8 * a);
    } else {
      const uint32_t m = n - p0 < kPerLane ? (uint32_t)(n - p0) : kPerLane;
      for (uint32_t k = 0; k < m; k++) w[k >> 2] |= (uint32_t)data[p0 + k] << (8 * (k & 3));
    }
    unsigned long long b0, b1;
    bytes_equal16(w, Rules::kFirst, b0, b1);
    unsigned long long f0 = b0, f1 = b1;
    if constexpr (Rules::kSecond != 0) {  // the sixteenth position: kFirst alone, its neighbour is another lane's
      unsigned long long l0, l1;
      bytes_equal16(w, Rules::kSecond, l0, l1);
      f0 = b0 & ((l0 >> 8) | (l1 << 56));
      f1 = b1 & ((l1 >> 8) | 0x8000000000000000ull);
    }
    while (f0 | f1) {
      uint32_t k;
      if (f0) {
        k = (uint32_t)(__ffsll((long long)f0) - 1) >> 3;
        f0 &= f0 - 1;
      } else {
        k = 8 + ((uint32_t)(__ffsll((long long)f1) - 1) >> 3);
        f1 &= f1 - 1;
      }
      const uint64_t p = p0 + k;
      uint32_t H;
      uint64_t size;
      if (p < n && Rules::message(data + p, n - p, &H, &size)) mask |= 1u << k;
    }
  }
  // lanes 4j .. 4j + 3 hold positions [64 (g / 4), + 64)
  unsigned long long m = mask;
  m |= (unsigned long long)__shfl_down(mask, 1) << 16;
  m |= (unsigned long long)__shfl_down(mask, 2) << 32;
  m |= (unsigned long long)__shfl_down(mask, 3) << 48;
  if ((threadIdx.x & 3) == 0 && p0 < n) {
    words[g >> 2] = m;
    counts[g >> 2] = (uint32_t)__popcll(m);
  }
}

// A message's 20 digest bytes at d (no alignment: read as bytes) stored as
// the five dwords of a digest table's row.
__device__ __forceinline__ void store_digest(uint32_t* o, const uint8_t* d) {
#pragma unroll
  for (int j = 0; j < 5; j++)
    o[j] = (uint32_t)d[4 * j] | (uint32_t)d[4 * j + 1] << 8 | (uint32_t)d[4 * j + 2] << 16 |
           (uint32_t)d[4 * j + 3] << 24;
}

// The 64 bitmap bits from position q on (bits past the bitmap are 0).
__device__ __forceinline__ unsigned long long bits_from(const unsigned long long* __restrict__ words, uint64_t nw,
                                                        uint64_t q) {
  const uint64_t w = q >> 6;
  const uint32_t s = (uint32_t)(q & 63);
  unsigned long long v = w < nw ? words[w] >> s : 0ull;
  if (s && w + 1 < nw) v |= words[w + 1] << (64 - s);
  return v;
}

__device__ __forceinline__ unsigned long long low_bits(uint32_t k) {  // k in 0..64
  return k >= 64 ? ~0ull : (1ull << k) - 1;
}

// The parsed sizes are 32 bits wide and their running offsets 64: the scans
// over them read through a transform iterator of this.
struct Widen {
  __host__ __device__ uint64_t operator()(uint32_t v) const { return (uint64_t)v; }
};

// What scan_candidates leaves in stream-ordered scratch, which goes back
// when this goes out of scope.
struct Scan {
  sfi::Scratch ws;
  uint64_t nw = 0;                      // bitmap words: ceil(n / 64)
  void* result = nullptr;               // 256 bytes for the caller's Result: zero, but its first 8 all ones
  unsigned long long* words = nullptr;  // [nw] bit k of word w: position 64 w + k is a candidate
  uint64_t* ends = nullptr;             // [nw] the candidates in words 0 .. w
  uint32_t* counts = nullptr;           // [nw] the candidates in word w
  explicit Scan(hipStream_t s) : ws(s) {}
};

// Candidates and scan of d_wire[0, n) (n > 0) on s.  Asynchronous.  The
// first 8 bytes of the result area are the first_bad of both parsers, which
// their kernels lower with atomicMin.
template <class Rules>
int scan_candidates(const uint8_t* d_wire, uint64_t n, hipStream_t s, Scan* out) {
  using namespace sfi;
  const uint64_t nw = ceil_div(n, 64);
  size_t tmp = 0;
  int rc = scan_inclusive(nullptr, tmp, static_cast<uint32_t*>(nullptr), static_cast<uint64_t*>(nullptr), nw, s);
  if (rc != SF_OK) return rc;
  ScratchLayout L;
  const size_t result_at = L.add(256), words_at = L.add(nw * 8), ends_at = L.add(nw * 8), counts_at = L.add(nw * 4);
  if ((rc = stream_alloc(&out->ws.p, L.total() + tmp + 8, s)) != SF_OK) return rc;
  void* base = out->ws.p;
  out->nw = nw;
  out->result = L.at<void>(base, result_at);
  out->words = L.at<unsigned long long>(base, words_at);
  out->ends = L.at<uint64_t>(base, ends_at);
  out->counts = L.at<uint32_t>(base, counts_at);
  SF_HIP(hipMemsetAsync(out->result, 0, 256, s));
  SF_HIP(hipMemsetAsync(out->result, 0xFF, 8, s));
  rc = launch(candidates_kernel<Rules>, dim3((unsigned)ceil_div(n, 256 * kPerLane)), dim3(256), s, d_wire, n,
              out->words, out->counts);
  if (rc != SF_OK) return rc;
  return scan_inclusive(L.at<void>(base, L.total()), tmp, out->counts, out->ends, nw, s);
}

// The run wire[0, n_bytes) (n_bytes > 0) to HBM through the lease's two
// pinned stages, on s with the lease's events; *d_wire = where it lies.
// Returns when the last piece has arrived.
inline int upload_run(sfi::HostLease& res, const uint8_t* wire, uint64_t n_bytes, hipStream_t s, hipEvent_t* ev,
                      const uint8_t** d_wire) {
  using namespace sfi;
  void* d = nullptr;
  int rc = res.dev(kSlotFileTable, n_bytes, &d);
  if (rc != SF_OK) return rc;
  const uint64_t piece = std::min(n_bytes, kUploadPiece);
  void* pin[2] = {nullptr, nullptr};
  for (int b = 0; b < 2; b++)
    if ((rc = res.pin(kSlotData + b, piece, &pin[b])) != SF_OK) return rc;
  *d_wire = static_cast<const uint8_t*>(d);
  return two_stage(
      ceil_div(n_bytes, piece),
      [&](uint64_t k, int b) {
        const uint64_t o = k * piece, m = std::min(piece, n_bytes - o);
        memcpy(pin[b], wire + o, m);
        SF_HIP(hipMemcpyAsync(static_cast<uint8_t*>(d) + o, pin[b], m, hipMemcpyHostToDevice, s));
        SF_HIP(hipEventRecord(ev[b], s));
        return SF_OK;
      },
      [&](uint64_t, int b) {
        SF_HIP(hipEventSynchronize(ev[b]));
        return SF_OK;
      });
}

}  // namespace sfrs
