// sf_wire.hip -- FILE_BLOCK runs built on the device, of a fixed tiling and of
// an explicit block list (its own translation unit and code object: byte
// stores and a rocprim scan, no SHA-1).
//
// The reference's source streams one FILE_BLOCK message per block after
// FILE_START (src/sync/fs.rs:217-233, written by write_message,
// src/sync/ssh/proto.rs:162-166): "FILE_BLOCK\n" + the 20 raw digest bytes +
// "\n" + the block's size in decimal + "\n".  With the reference's default,
// content-defined blocks every size differs, so message i starts at the sum
// of the earlier messages' lengths (33 + digits(size)): one pass writes the
// lengths, a rocprim inclusive scan turns them into end offsets, and one
// thread per message writes it at its place.  In a fixed tiling every block
// is block_size bytes except the last, so message i starts at
// i * (33 + digits(block_size)) and one kernel writes the run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sf_device.hpp"
#include "sf_launch.hpp"

namespace {

// Decimal digits of v, on the device and on the host.  The division runs in
// v's own width: the explicit-list kernels divide in 32 bits, the fixed
// tiling's kernel widens its argument and divides in 64, which is how each
// was compiled when its machine code was recorded.
template <typename T>
__host__ __device__ __forceinline__ uint32_t digits10(T v) {
  uint32_t d = 1;
  while (v >= 10) { v /= 10; ++d; }
  return d;
}

__global__ void __launch_bounds__(256) wire_len_kernel(const uint32_t* __restrict__ sizes, uint64_t n,
                                                       uint64_t* __restrict__ lens) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) lens[i] = 33u + digits10(sizes[i]);  // 11 + 20 + 1 + digits + 1
}

// Message i goes to out + ends[i] - base - its length (base: the end offset
// of the message before the first one written, so a chunk of a longer run
// lands at the start of its own buffer).
__global__ void __launch_bounds__(256) wire_blocks_kernel(const uint8_t* __restrict__ digests,
                                                          const uint32_t* __restrict__ sizes,
                                                          const uint64_t* __restrict__ ends, uint64_t n,
                                                          uint64_t base, uint8_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t v = sizes[i];
  const uint32_t nd = digits10(v);
  uint8_t* o = out + (ends[i] - base) - (33u + nd);
  const char tag[11] = {'F', 'I', 'L', 'E', '_', 'B', 'L', 'O', 'C', 'K', '\n'};
#pragma unroll
  for (int k = 0; k < 11; ++k) o[k] = (uint8_t)tag[k];
  const uint8_t* d = digests + i * 20;
#pragma unroll
  for (int k = 0; k < 20; ++k) o[11 + k] = d[k];
  o[31] = '\n';
  for (int k = (int)nd - 1; k >= 0; --k) { o[32 + k] = (uint8_t)('0' + v % 10); v /= 10; }
  o[32 + nd] = '\n';
}

// out[k] = ends[min((k + 1) * per, n) - 1]: the end offset of chunk k
__global__ void __launch_bounds__(256) wire_chunk_ends_kernel(const uint64_t* __restrict__ ends, uint64_t n,
                                                              uint64_t per, uint64_t nchunks,
                                                              uint64_t* __restrict__ out) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < nchunks) out[k] = ends[std::min((k + 1) * per, n) - 1];
}

constexpr uint64_t kWireMaxPerLaunch = 1ull << 30;  // messages per launch (grid x stays far below 2^31)

}  // namespace

namespace sf {

// The FILE_BLOCK messages of a fixed tiling.  One thread per message, byte
// stores.
__global__ void __launch_bounds__(256)
wire_file_blocks_kernel(const uint8_t* __restrict__ digests, uint64_t n, uint32_t block_size, uint32_t last_size,
                        uint8_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t db = digits10((uint64_t)block_size);
  const uint64_t msg = 33 + db;  // 11 + 20 + 1 + digits + 1
  uint8_t* o = out + i * msg;
  const char tag[11] = {'F', 'I', 'L', 'E', '_', 'B', 'L', 'O', 'C', 'K', '\n'};
#pragma unroll
  for (int k = 0; k < 11; ++k) o[k] = (uint8_t)tag[k];
  const uint8_t* d = digests + i * 20;
#pragma unroll
  for (int k = 0; k < 20; ++k) o[11 + k] = d[k];
  o[31] = '\n';
  uint32_t v = (i + 1 == n) ? last_size : block_size;
  const uint32_t nd = digits10((uint64_t)v);
  for (int k = (int)nd - 1; k >= 0; --k) { o[32 + k] = (uint8_t)('0' + v % 10); v /= 10; }
  o[32 + nd] = '\n';
}

}  // namespace sf

namespace sfi {

int launch_wire(const uint8_t* d_digests, uint64_t n, uint32_t bs, uint32_t last, uint8_t* d_out,
                hipStream_t stream) {
  if (n == 0) return SF_OK;
  const uint64_t maxb = launch_max_blocks();
  if (n > maxb) {  // consecutive runs of messages, one launch each
    for (uint64_t first = 0; first < n; first += maxb) {
      const uint64_t cnt = std::min(maxb, n - first);
      const int rc = launch_wire(d_digests + first * 20, cnt, bs, first + cnt == n ? last : bs,
                                 d_out + first * (33 + digits10(bs)), stream);
      if (rc) return rc;
    }
    return SF_OK;
  }
  return launch(sf::wire_file_blocks_kernel, grid256(n), dim3(256), stream, d_digests, n, bs, last, d_out);
}

// The end offset of every message of the run (inclusive scan of the
// lengths), in stream-ordered scratch the caller frees with stream_free on
// `s`.
int wire_plan(const uint32_t* d_sizes, uint64_t n, uint64_t** d_ends, hipStream_t s) {
  *d_ends = nullptr;
  size_t tmp = 0;
  uint64_t* const nul = nullptr;
  int rc = scan_inclusive(nullptr, tmp, nul, nul, n, s);
  if (rc != SF_OK) return rc;
  // ends first (returned), then lengths and the scan's temporary
  ScratchLayout L;
  const size_t ends_at = L.add(n * 8), lens_at = L.add(n * 8);
  void* ws = nullptr;
  if ((rc = stream_alloc(&ws, L.total() + tmp + 8, s)) != SF_OK) return rc;
  uint64_t* ends = L.at<uint64_t>(ws, ends_at);
  uint64_t* lens = L.at<uint64_t>(ws, lens_at);
  // pieces of at most 2^30 messages per launch: a grid past 2^32 work-items
  // is not launched whole
  rc = for_pieces(n, kWireMaxPerLaunch, [&](uint64_t first, uint64_t cnt) {
    return launch(wire_len_kernel, grid256(cnt), dim3(256), s, d_sizes + first, cnt, lens + first);
  });
  if (rc == SF_OK) rc = scan_inclusive(L.at<void>(ws, L.total()), tmp, lens, ends, n, s);
  if (rc != SF_OK) {
    stream_free(ws, s);
    return rc;
  }
  *d_ends = ends;
  return SF_OK;
}

// d_chunk_ends[k] = end offset of chunk k (chunks of `per` messages).
int wire_chunk_ends(const uint64_t* d_ends, uint64_t n, uint64_t per, uint64_t* d_chunk_ends, hipStream_t s) {
  const uint64_t nchunks = ceil_div(n, per);
  return launch(wire_chunk_ends_kernel, grid256(nchunks), dim3(256), s, d_ends, n, per, nchunks, d_chunk_ends);
}

// Messages [first, first + cnt) of a planned run, written from the start of
// d_out (base = the end offset of message first - 1, 0 for the first).
int wire_build(const uint8_t* d_digests, const uint32_t* d_sizes, const uint64_t* d_ends, uint64_t first,
               uint64_t cnt, uint64_t base, uint8_t* d_out, hipStream_t s) {
  return for_pieces(cnt, kWireMaxPerLaunch, [&](uint64_t a, uint64_t m) {
    return launch(wire_blocks_kernel, grid256(m), dim3(256), s, d_digests + (first + a) * 20, d_sizes + first + a,
                  d_ends + first + a, m, base, d_out);
  });
}

}  // namespace sfi

extern "C" {

int sf_wire_file_blocks_device(const void* d_digests, uint64_t n_blocks, uint32_t block_size, uint64_t file_len,
                               void* d_out, uint64_t cap, uint64_t* n_out, void* stream) {
  using sfi::ceil_div;
  if (block_size == 0 || block_size > SF_MAX_BLOCK_SIZE) return SF_EINVAL;
  const uint64_t nb = file_len ? ceil_div(file_len, block_size) : 0;
  if (nb != n_blocks) return SF_EINVAL;
  const uint32_t last = nb ? (uint32_t)(file_len - (nb - 1) * block_size) : 0;
  const uint64_t bytes = nb ? (nb - 1) * (33 + (uint64_t)digits10(block_size)) + (33 + digits10(last)) : 0;
  if (n_out) *n_out = bytes;
  if (bytes > cap) return SF_ENOSPC;
  if (!nb) return SF_OK;
  if (!d_digests || !d_out) return SF_EINVAL;
  return sfi::launch_wire(static_cast<const uint8_t*>(d_digests), nb, block_size, last, static_cast<uint8_t*>(d_out),
                          sfi::as_stream(stream));
}

int sf_wire_blocks_device(const void* d_digests, const uint32_t* d_sizes, uint64_t n_blocks, void* d_out,
                          uint64_t cap, uint64_t* n_out, void* stream) {
  using sfi::ceil_div;
  if (n_out) *n_out = 0;
  if (n_blocks == 0) return SF_OK;
  if (!d_sizes) return SF_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  uint64_t* ends = nullptr;
  int rc = sfi::wire_plan(d_sizes, n_blocks, &ends, s);
  if (rc != SF_OK) return rc;
  uint64_t total = 0;
  do {
    // the need is the last end offset: read back (this call blocks here)
    if (hipMemcpyAsync(&total, ends + n_blocks - 1, 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
      rc = SF_ENODEV;
      break;
    }
    if (n_out) *n_out = total;
    if (total > cap || !d_out) { rc = SF_ENOSPC; break; }
    if (!d_digests) { rc = SF_EINVAL; break; }
    rc = sfi::wire_build(static_cast<const uint8_t*>(d_digests), d_sizes, ends, 0, n_blocks, 0,
                         static_cast<uint8_t*>(d_out), s);
  } while (0);
  sfi::stream_free(ends, s);
  return rc;
}

}  // extern "C"
