// sf_capi.hip -- the fixed-tiling kernel, the stand-alone chain kernel and the
// splitmix fill, with their launchers, and the simple device-resident entry
// points of the C-ABI (include/syncfast_amd.h).
//
// One of the library's GPU translation units (sf_internal.hpp lists them);
// its code object holds the three kernels named above.  sha1_fixed_kernel is
// the headline kernel: bench.py keys its roofline traffic on the hash of its
// machine code (profiles/traffic.json).  sha1_chain_kernel shares the object:
// compiled next to the helper-wave chain kernel of sf_chain.hip it came out
// 100 instructions longer.  There is no CPU implementation of the block
// hashing in this library: without a HIP device the entry points return
// SF_ENODEV.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "sf_block_hash.hpp"
#include "sf_device.hpp"

namespace sf {

// WPE = minimum resident waves per SIMD requested from the register
// allocator (__launch_bounds__ 2nd argument, per EU on gfx950).
template <int TILE, int WPE = 1, bool WEAK = false>
__global__ void __launch_bounds__(kThreads, WPE)
sha1_fixed_kernel(const uint8_t* __restrict__ data, uint64_t len, uint32_t bs, uint64_t nblocks,
                  uint8_t* __restrict__ digests, const PadSchedule pad, uint32_t* __restrict__ weak) {
  __shared__ uint4 smem[kWavesPerWG * 64 * (TILE / 16)];
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform -> SGPR
  fixed_wave<TILE, WEAK>(data, len, bs, nblocks, digests, pad, weak, (uint64_t)blockIdx.x * kWavesPerWG + wid,
                         smem + wid * 64 * (TILE / 16));
}

// Stream a 64-B-multiple byte range [lo, hi) of a lane's message through
// SHA-1, the next chunk's loads issued before each compression (the load
// has a whole compression to land; one register set keeps the VGPR count
// under the block kernel's when fused with it).
__device__ __forceinline__ void sha1_stream_range(Sha1& st, const uint4* __restrict__ q, uint32_t lo, uint32_t hi) {
  if (lo + 64 > hi) return;
  uint4 c0 = q[lo / 16], c1 = q[lo / 16 + 1], c2 = q[lo / 16 + 2], c3 = q[lo / 16 + 3];
  for (uint32_t c = lo; c + 64 <= hi; c += 64) {
    const uint32_t nx = (c + 128 <= hi) ? (c + 64) / 16 : c / 16;
    const uint4 n0 = q[nx], n1 = q[nx + 1], n2 = q[nx + 2], n3 = q[nx + 3];
    __builtin_amdgcn_sched_barrier(0);
    uint32_t w[16] = {bswap32(c0.x), bswap32(c0.y), bswap32(c0.z), bswap32(c0.w),
                      bswap32(c1.x), bswap32(c1.y), bswap32(c1.z), bswap32(c1.w),
                      bswap32(c2.x), bswap32(c2.y), bswap32(c2.z), bswap32(c2.w),
                      bswap32(c3.x), bswap32(c3.y), bswap32(c3.z), bswap32(c3.w)};
    st.compress(w);
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
  }
}

// One lane per file: the file's blocks_hash (src/index.rs:661-682) = SHA-1
// over its run of run_len digest bytes (the stand-alone chain kernel).
__device__ __forceinline__ void chain_wave(const uint8_t* __restrict__ runs, uint64_t run_stride, uint32_t f,
                                           bool valid, uint32_t run_len, uint8_t* __restrict__ out) {
  if (!valid) return;
  Sha1 st;
  st.init();
  const uint8_t* p = runs + (uint64_t)f * run_stride;
  sha1_stream_range(st, reinterpret_cast<const uint4*>(p), 0, (run_len / 64) * 64);
  const uint32_t nch = n_chunks(run_len);
  for (uint32_t c = run_len / 64; c < nch; ++c) {
    uint32_t w[16];
    build_tail_chunk(w, p, run_len, c, nch);
    st.compress(w);
  }
  st.store(out + (uint64_t)f * 20);
}

// Stand-alone chains (no stages): one lane per file over its whole run.
__global__ void __launch_bounds__(64)
sha1_chain_kernel(const uint8_t* __restrict__ runs, uint64_t run_stride, uint32_t nfiles, uint32_t run_len,
                  uint8_t* __restrict__ out) {
  const uint32_t f = blockIdx.x * 64 + threadIdx.x;
  chain_wave(runs, run_stride, f, f < nfiles, run_len, out);
}

// splitmix64 byte stream: word i = mix(seed + (i+1)*GAMMA),
// little-endian; writes bytes [start, start+len) of the stream.
__device__ __forceinline__ uint64_t splitmix_word(uint64_t seed, uint64_t i) {
  uint64_t z = seed + (i + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__global__ void __launch_bounds__(256)
fill_splitmix_kernel(uint8_t* __restrict__ out, uint64_t len, uint64_t seed, uint64_t start) {
  // Fast path: whole 16-B groups of 2 aligned stream words.
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  if ((start & 15u) == 0 && (reinterpret_cast<uintptr_t>(out) & 15u) == 0) {
    const uint64_t nvec = len / 16;
    const uint64_t w0 = start / 8;
    for (uint64_t v = tid; v < nvec; v += stride) {
      const uint64_t a = splitmix_word(seed, w0 + 2 * v), b = splitmix_word(seed, w0 + 2 * v + 1);
      reinterpret_cast<ulonglong2*>(out)[v] = make_ulonglong2(a, b);
    }
    for (uint64_t p = nvec * 16 + tid; p < len; p += stride) {
      const uint64_t sp = start + p;
      out[p] = (uint8_t)(splitmix_word(seed, sp >> 3) >> (8 * (sp & 7)));
    }
  } else {
    for (uint64_t p = tid; p < len; p += stride) {
      const uint64_t sp = start + p;
      out[p] = (uint8_t)(splitmix_word(seed, sp >> 3) >> (8 * (sp & 7)));
    }
  }
}

}  // namespace sf

namespace sfi {

constexpr int kTile = 128;  // bytes of each block staged per LDS step

uint64_t launch_max_blocks() {
  const int64_t v = knob(K_TEST_LAUNCH_MAX_BLOCKS);
  return v > 0 ? std::max<uint64_t>(16, (uint64_t)v & ~15ull) : (1ull << 31);
}

int launch_fixed(const void* d_data, uint64_t len, uint32_t bs, uint64_t nblocks, void* d_digests,
                 hipStream_t stream, uint32_t* weak) {
  if (nblocks == 0) return SF_OK;
  const uint64_t maxb = launch_max_blocks();
  if (nblocks > maxb) {  // consecutive pieces of the tiling, one launch each
    for (uint64_t first = 0; first < nblocks; first += maxb) {
      const uint64_t cnt = std::min(maxb, nblocks - first), off = first * (uint64_t)bs;
      const int rc = launch_fixed(static_cast<const uint8_t*>(d_data) + off, std::min(len - off, cnt * (uint64_t)bs),
                                  bs, cnt, static_cast<uint8_t*>(d_digests) + first * 20, stream,
                                  weak ? weak + first : nullptr);
      if (rc) return rc;
    }
    return SF_OK;
  }
  const unsigned grid = (unsigned)ceil_div(ceil_div(nblocks, 64), sf::kWavesPerWG);
  const sf::PadSchedule pad = pad_schedule(bs);
  const uint8_t* d = static_cast<const uint8_t*>(d_data);
  uint8_t* o = static_cast<uint8_t*>(d_digests);
  if (weak)  // opt-in fused Adler-32 (a separate instantiation; the default kernel is unchanged)
    return launch(sf::sha1_fixed_kernel<kTile, 1, true>, dim3(grid), dim3(sf::kThreads), stream, d, len, bs, nblocks, o,
                  pad, weak);
  return launch(sf::sha1_fixed_kernel<kTile, 1>, dim3(grid), dim3(sf::kThreads), stream, d, len, bs, nblocks, o, pad,
                nullptr);
}

int launch_chain_plain(const uint8_t* d_runs, uint64_t run_stride, uint32_t nfiles, uint32_t run_len,
                       uint8_t* d_hashes, hipStream_t stream) {
  return launch(sf::sha1_chain_kernel, dim3((unsigned)ceil_div(nfiles, 64)), dim3(64), stream, d_runs, run_stride,
                nfiles, run_len, d_hashes);
}

// The fixed-tiling entry point and its weak form: d_weak is asked for and
// checked only when want_weak.
static int index_device_fixed(const void* d_data, uint64_t len, uint32_t block_size, void* d_digests,
                              uint32_t* d_weak, bool want_weak, uint64_t cap_blocks, uint64_t* n_blocks,
                              void* stream) {
  int rc = check_block_size(block_size);
  if (rc) return rc;
  // digests (and weak sums) are written as dwords (Sha1::store)
  if (misaligned(d_digests, 4) || misaligned(d_weak, 4)) return SF_EINVAL;
  const uint64_t nb = len ? ceil_div(len, block_size) : 0;
  if (n_blocks) *n_blocks = nb;
  if (nb > cap_blocks) return SF_ENOSPC;
  if (nb && (!d_data || !d_digests || (want_weak && !d_weak))) return SF_EINVAL;
  return launch_fixed(d_data, len, block_size, nb, d_digests, as_stream(stream), d_weak);
}

// The explicit-list entry point and its weak form.
static int index_device_blocks(const void* d_data, uint64_t len, const uint64_t* d_offsets, const uint32_t* d_sizes,
                               uint64_t n_blocks, void* d_digests, uint32_t* d_weak, bool want_weak, int* d_status,
                               void* stream) {
  if (n_blocks == 0) return SF_OK;
  // d_data may be NULL only when len == 0 (then every in-range block is
  // empty and the kernel dereferences nothing).
  if (!d_offsets || !d_sizes || !d_digests || (want_weak && !d_weak) || (!d_data && len)) return SF_EINVAL;
  // digests are written, and an out-of-range block's zeroed, as dwords
  if (misaligned(d_digests, 4) || misaligned(d_weak, 4) || misaligned(d_status, 4)) return SF_EINVAL;
  return launch_table(d_data, len, d_offsets, d_sizes, n_blocks, d_digests, d_status, as_stream(stream), d_weak);
}

}  // namespace sfi

using namespace sfi;

extern "C" {

const char* sf_version(void) { return "syncfast_amd 0.1.0 (gfx950)"; }

const char* sf_strerror(int code) {
  switch (code) {
    case SF_OK: return "ok";
    case SF_EIO: return "I/O error";
    case SF_EAGAIN: return "the file changed while it was indexed (cut it again and retry)";
    case SF_ENOMEM: return "out of memory";
    case SF_ENODEV: return "no HIP device or HIP runtime error";
    case SF_EINVAL: return "invalid argument";
    case SF_ENOSPC: return "output capacity too small";
    case SF_ERANGE: return "block outside the input";
    case SF_ETIMEDOUT: return "device-side wait timed out (no longer returned)";
    default: return "unknown error";
  }
}

int sf_device_count(int* n) {
  if (!n) return SF_EINVAL;
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
  *n = c;
  return SF_OK;
}

int sf_set_device(int device) { return hip_err(hipSetDevice(device)); }

int sf_index_device_fixed(const void* d_data, uint64_t len, uint32_t block_size, void* d_digests,
                          uint64_t cap_blocks, uint64_t* n_blocks, void* stream) {
  return index_device_fixed(d_data, len, block_size, d_digests, nullptr, false, cap_blocks, n_blocks, stream);
}

int sf_index_device_fixed_weak(const void* d_data, uint64_t len, uint32_t block_size, void* d_digests,
                               uint32_t* d_weak, uint64_t cap_blocks, uint64_t* n_blocks, void* stream) {
  return index_device_fixed(d_data, len, block_size, d_digests, d_weak, true, cap_blocks, n_blocks, stream);
}

int sf_index_device_blocks(const void* d_data, uint64_t len, const uint64_t* d_offsets, const uint32_t* d_sizes,
                           uint64_t n_blocks, void* d_digests, int* d_status, void* stream) {
  return index_device_blocks(d_data, len, d_offsets, d_sizes, n_blocks, d_digests, nullptr, false, d_status, stream);
}

int sf_index_device_blocks_weak(const void* d_data, uint64_t len, const uint64_t* d_offsets, const uint32_t* d_sizes,
                                uint64_t n_blocks, void* d_digests, uint32_t* d_weak, int* d_status, void* stream) {
  return index_device_blocks(d_data, len, d_offsets, d_sizes, n_blocks, d_digests, d_weak, true, d_status, stream);
}

int sf_fill_splitmix_device(void* d_out, uint64_t len, uint64_t seed, uint64_t start, void* stream) {
  if (len == 0) return SF_OK;
  if (!d_out) return SF_EINVAL;
  const uint64_t nvec = len / 16 + 1;
  const unsigned grid = (unsigned)std::min<uint64_t>(ceil_div(nvec, 256), 65536);
  return launch(sf::fill_splitmix_kernel, dim3(grid), dim3(256), as_stream(stream), static_cast<uint8_t*>(d_out), len,
                seed, start);
}

}  // extern "C"
