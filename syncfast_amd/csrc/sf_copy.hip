// sf_copy.hip -- the block copy kernel (include/syncfast_amd.h:
// sf_copy_blocks_device): job i moves size[i] bytes from src + src_off[i] to
// dst + dst_off[i], nothing aligned, every job of a call in one launch.  What
// the sink states of the reference do with read_block / write_block per block
// (src/sync/fs.rs:463-470, 505-510), for a whole copy or write list at once,
// from HBM to HBM.  Its own translation unit: the other kernels' code objects
// stay as they are.  The arithmetic is sf_copy_plan.hpp's, shared with the
// host test that executes it.
//
// Work is split by bytes, not by jobs: a job is cut into tiles of T = 4 KiB on
// T-aligned destination addresses, so one job of 4 GiB and a million jobs of
// one byte both spread over the chip.  The steps, ordered by kernel
// boundaries only (no lane waits for another wave, nothing is read back):
//
//   count   one lane per job: the job is copied when it is taken, its source
//           lies in [0, src_len) and its destination in [0, dst_len); a taken
//           job that is not sets *d_status.  Its tile count (0 when it is not
//           copied, or empty) goes to P[i + 1]; P[0] = 0.
//   scan    rocprim inclusive scan of P[1 .. n] in place, uint64: P[i] = the
//           first tile of job i, P[n] = the tiles of the call.
//   copy    a grid sized from the CU count.  A wave takes runs of kRun
//           consecutive tiles in a grid-stride loop: one binary search of P
//           for the run's first tile, then it walks on through P.  A tile is
//           written by one wave: the up to 15 bytes before the first 16-byte
//           boundary of the destination and the up to 15 after the last by
//           byte stores (a job's first and last tile only), everything
//           between by 16-byte stores aligned in the destination, a lane
//           taking up to four of them.  No store touches a byte outside its
//           job's range: neighbours that abut byte to byte are written by
//           other waves at the same time, and a dword or a line read, merged
//           and written back at an edge would undo their bytes.  The source
//           bytes of a 16-byte store come as four or five aligned dwords
//           funnel-shifted by (src - dst) & 3, byte by byte where those
//           dwords would leave [d_src, d_src + src_len).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sf_copy_plan.hpp"
#include "sf_device.hpp"
#include "../../include/syncfast_amd_test.h"

namespace {

constexpr uint64_t kMaxJobs = 1ull << 32;  // the count kernel's grid stays below 2^31 workgroups
constexpr uint32_t kRun = 8;               // consecutive tiles a wave takes per search (32 KiB)
constexpr uint32_t kWalk = 8;              // jobs a wave steps over in P before it searches again
constexpr uint32_t kWavesPerBlock = 4;
constexpr uint32_t kBlocksPerCU = 8;

// What the device keeps of the last call for sf_test_copy_stats.
struct DevStats {
  unsigned long long copied, tiles;
};

__global__ void __launch_bounds__(256) copy_count_kernel(const uint64_t* __restrict__ src_off,
                                                         const uint64_t* __restrict__ dst_off,
                                                         const uint32_t* __restrict__ sizes,
                                                         const uint8_t* __restrict__ take, uint64_t n, uint64_t src_len,
                                                         uint64_t dst, uint64_t dst_len, uint64_t* __restrict__ P,
                                                         int* __restrict__ status, DevStats* __restrict__ stats) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) P[0] = 0;
  bool copied = false;
  if (i < n) {
    const bool taken = !take || take[i];
    const uint64_t so = src_off[i], dof = dst_off[i];
    const uint32_t size = sizes[i];
    copied = taken && sfcp::in_range(so, size, src_len) && sfcp::in_range(dof, size, dst_len);
    if (taken && !copied && status) *status = SF_ERANGE;
    P[i + 1] = copied ? sfcp::tile_count(dst + dof, size) : 0;
  }
  const uint32_t c = (uint32_t)__popcll(__ballot(copied));
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(&stats->copied, (unsigned long long)c);
}

// The largest j in [lo, n) with P[j] <= t, given P[lo] <= t < P[n].  Job j
// then holds tile t: P[j + 1] > t.
__device__ __forceinline__ uint64_t find_job(const uint64_t* __restrict__ P, uint64_t lo, uint64_t n, uint64_t t) {
  uint64_t hi = n;
  while (hi - lo > 1) {
    const uint64_t m = lo + ((hi - lo) >> 1);
    if (P[m] <= t) lo = m;
    else hi = m;
  }
  return lo;
}

// The 16 source bytes at address s as four little-endian dwords; `src` is the
// buffer at addresses [lo, hi).
__device__ __forceinline__ uint4 load_chunk(const uint8_t* __restrict__ src, uint64_t lo, uint64_t hi, uint64_t s) {
  const sfcp::Load L = sfcp::chunk_load(s, lo, hi);
  uint4 v;
  if (L.dwords) {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(src + (L.at - lo));
    const uint32_t d0 = p[0], d1 = p[1], d2 = p[2], d3 = p[3];
    const uint32_t d4 = L.shift ? p[4] : 0u;
    const uint32_t sh = 8 * L.shift;
    v.x = __funnelshift_r(d0, d1, sh);
    v.y = __funnelshift_r(d1, d2, sh);
    v.z = __funnelshift_r(d2, d3, sh);
    v.w = __funnelshift_r(d3, d4, sh);
  } else {
    const uint8_t* q = src + (s - lo);
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) w[k >> 2] |= (uint32_t)q[k] << (8 * (k & 3));
    v = make_uint4(w[0], w[1], w[2], w[3]);
  }
  return v;
}

__global__ void __launch_bounds__(64 * kWavesPerBlock) copy_tiles_kernel(
    const uint8_t* __restrict__ src, uint64_t src_len, uint8_t* __restrict__ dst,
    const uint64_t* __restrict__ src_off, const uint64_t* __restrict__ dst_off, const uint32_t* __restrict__ sizes,
    const uint64_t* __restrict__ P, uint64_t n, DevStats* __restrict__ stats) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = (uint64_t)blockIdx.x * kWavesPerBlock + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t nwaves = (uint64_t)gridDim.x * kWavesPerBlock;
  const uint64_t total = P[n];
  if (wave == 0 && lane == 0) stats->tiles = total;
  const uint64_t slo = reinterpret_cast<uint64_t>(src), shi = slo + src_len;
  const uint64_t dlo = reinterpret_cast<uint64_t>(dst);
  for (uint64_t t0 = wave * kRun; t0 < total; t0 += nwaves * kRun) {
    const uint64_t t_end = t0 + kRun < total ? t0 + kRun : total;
    uint64_t j = find_job(P, 0, n, t0);
    uint64_t t = t0;
    while (t < t_end) {
      // on to the job that holds tile t: the next few entries, else a search
      for (uint32_t w = 0; w < kWalk && P[j + 1] <= t; w++) j++;
      if (P[j + 1] <= t) j = find_job(P, j + 1, n, t);
      const uint64_t first = P[j], next = P[j + 1];
      const uint64_t D = dlo + dst_off[j];
      const uint64_t delta = (slo + src_off[j]) - D;  // source address - destination address, mod 2^64
      const uint32_t size = sizes[j];
      const uint64_t stop = next < t_end ? next : t_end;
      for (; t < stop; t++) {
        const sfcp::Tile tr = sfcp::tile_range(D, size, t - first);
        const sfcp::Split sp = sfcp::split(tr.a, tr.e);
        // edges: lanes 0..14 the head, lanes 32..46 the tail, a byte each
        const uint32_t hn = (uint32_t)(sp.h - tr.a), tn = (uint32_t)(tr.e - sp.b);
        if (lane < hn) dst[tr.a + lane - dlo] = src[tr.a + lane + delta - slo];
        if (lane >= 32 && lane - 32 < tn) dst[sp.b + (lane - 32) - dlo] = src[sp.b + (lane - 32) + delta - slo];
        // body: chunk c at destination address sp.h + 16 c, all loads before the stores
        const uint32_t chunks = (uint32_t)((sp.b - sp.h) / sfcp::kVec);
        uint4 v[sfcp::kTileChunks / 64];
#pragma unroll
        for (uint32_t r = 0; r < sfcp::kTileChunks / 64; r++) {
          const uint32_t c = lane + 64 * r;
          if (c < chunks) v[r] = load_chunk(src, slo, shi, sp.h + sfcp::kVec * c + delta);
        }
#pragma unroll
        for (uint32_t r = 0; r < sfcp::kTileChunks / 64; r++) {
          const uint32_t c = lane + 64 * r;
          if (c < chunks) *reinterpret_cast<uint4*>(dst + (sp.h + sfcp::kVec * c - dlo)) = v[r];
        }
      }
    }
  }
}

std::atomic<uint64_t> g_copy_launches{0};
std::atomic<int> g_copy_dev{-1};  // the device of the last call that launched
std::atomic<void*> g_dev_stats[sfi::kMaxDevices];
std::atomic<int> g_cus[sfi::kMaxDevices];

}  // namespace

using namespace sfi;

namespace {

// This device's CU count and its DevStats (allocated once, never freed: the
// runtime may be gone when a static destructor runs).
int device_state(int* dev, int* cus, DevStats** stats) {
  SF_HIP(hipGetDevice(dev));
  if (*dev < 0 || *dev >= kMaxDevices) return SF_ENODEV;
  int c = g_cus[*dev].load(std::memory_order_relaxed);
  if (c <= 0) {
    SF_HIP(hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, *dev));
    if (c <= 0) return SF_ENODEV;
    g_cus[*dev].store(c, std::memory_order_relaxed);
  }
  void* p = g_dev_stats[*dev].load(std::memory_order_acquire);
  if (!p) {
    void* q = nullptr;
    SF_HIP(hipMalloc(&q, 256));
    if (g_dev_stats[*dev].compare_exchange_strong(p, q, std::memory_order_acq_rel)) p = q;
    else (void)hipFree(q);
  }
  *cus = c;
  *stats = static_cast<DevStats*>(p);
  return SF_OK;
}

}  // namespace

int sfi::copy_blocks(const uint8_t* d_src, uint64_t src_len, uint8_t* d_dst, uint64_t dst_len,
                     const uint64_t* d_src_off, const uint64_t* d_dst_off, const uint32_t* d_sizes,
                     const uint8_t* d_take, uint64_t n, int* d_status, hipStream_t s) {
  g_copy_launches.store(0, std::memory_order_relaxed);
  g_copy_dev.store(-1, std::memory_order_relaxed);
  if (n == 0) return SF_OK;
  if (!d_src || !d_dst || !d_src_off || !d_dst_off || !d_sizes || n > kMaxJobs) return SF_EINVAL;
  if (misaligned(d_status, 4)) return SF_EINVAL;  // written as one int
  const uint64_t a = reinterpret_cast<uint64_t>(d_src), b = reinterpret_cast<uint64_t>(d_dst);
  if (src_len && dst_len && a < b + dst_len && b < a + src_len) return SF_EINVAL;  // the buffers overlap

  int dev = 0, cus = 0;
  DevStats* stats = nullptr;
  int rc = device_state(&dev, &cus, &stats);
  if (rc != SF_OK) return rc;
  size_t tmp = 0;
  uint64_t* const nul = nullptr;
  if ((rc = scan_inclusive(nullptr, tmp, nul, nul, n, s)) != SF_OK) return rc;
  ScratchLayout L;
  const size_t p_at = L.add((n + 1) * 8);
  Scratch ws(s);
  if ((rc = stream_alloc(&ws.p, L.total() + tmp + 8, s)) != SF_OK) return rc;
  uint64_t* P = L.at<uint64_t>(ws.p, p_at);
  SF_HIP(hipMemsetAsync(stats, 0, sizeof(DevStats), s));
  rc = launch(copy_count_kernel, grid256(n), dim3(256), s, d_src_off, d_dst_off, d_sizes, d_take, n, src_len, b,
              dst_len, P, d_status, stats);
  if (rc == SF_OK) rc = scan_inclusive(L.at<void>(ws.p, L.total()), tmp, P + 1, P + 1, n, s);
  if (rc == SF_OK)
    rc = launch(copy_tiles_kernel, dim3((unsigned)cus * kBlocksPerCU), dim3(64 * kWavesPerBlock), s, d_src, src_len,
                d_dst, d_src_off, d_dst_off, d_sizes, P, n, stats);
  if (rc != SF_OK) return rc;
  g_copy_launches.store(1, std::memory_order_relaxed);
  g_copy_dev.store(dev, std::memory_order_relaxed);
  return SF_OK;
}

extern "C" {

int sf_copy_blocks_device(const void* d_src, uint64_t src_len, void* d_dst, uint64_t dst_len,
                          const uint64_t* d_src_offsets, const uint64_t* d_dst_offsets, const uint32_t* d_sizes,
                          const uint8_t* d_take, uint64_t n_blocks, int* d_status, void* stream) {
  return guarded([&] {
    return copy_blocks(static_cast<const uint8_t*>(d_src), src_len, static_cast<uint8_t*>(d_dst), dst_len,
                       d_src_offsets, d_dst_offsets, d_sizes, d_take, n_blocks, d_status, as_stream(stream));
  });
}

int sf_test_copy_stats(uint64_t out[4]) {
  if (!out) return SF_EINVAL;
  out[0] = sfcp::kTile;
  out[1] = out[2] = 0;
  out[3] = g_copy_launches.load(std::memory_order_relaxed);
  const int dev = g_copy_dev.load(std::memory_order_relaxed);
  if (dev < 0) return SF_OK;  // the last call launched nothing
  int cur = 0;
  SF_HIP(hipGetDevice(&cur));
  if (cur != dev) SF_HIP(hipSetDevice(dev));
  DevStats h{};
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(&h, g_dev_stats[dev].load(std::memory_order_acquire), sizeof(h), hipMemcpyDeviceToHost);
  if (cur != dev) (void)hipSetDevice(cur);
  if (e != hipSuccess) return hip_err(e);
  out[1] = h.copied;
  out[2] = h.tiles;
  return SF_OK;
}

}  // extern "C"
