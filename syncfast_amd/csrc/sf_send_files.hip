// sf_send_files.hip -- the source's answer to a whole list of GET_FILE
// requests, built on the device in one call (include/syncfast_amd.h:
// sf_wire_files_device).  The reference's source answers file after file:
// FILE_START with the name, one FILE_BLOCK per block, FILE_END
// (src/sync/fs.rs:177-231, written by write_message,
// src/sync/ssh/proto.rs:157-169).  The receiving half is
// sf_recv_files.hip; this is the sending half.  Its own translation unit: the
// other kernels' code objects stay as they are.  The framing rules, the
// places of the messages and the per-file test are sf_wire_send_files.hpp's,
// shared with the host test that executes them.
//
// The files are two CSRs, first[] over the block table and name_at[] over the
// packed names.  Ordered by kernel boundaries only (no lane waits for another
// wave):
//
//   plan   sfi::wire_plan (sf_wire.hip): the FILE_BLOCK lengths and their
//          inclusive scan E, as for one file's run.
//   check  one lane per file: file_ok of its entries and its name; the
//          smallest failing file is an atomicMin, one per wave.  The last
//          file's lane puts E's last entry and name_at[n_files] beside that
//          word, and the three come back in one 24-byte copy: the call's only
//          read-back.  The run is allocated then.
//   files  one lane per file: FILE_START with the name's bytes at start_at(f),
//          FILE_END at end_at(f), byte stores.
//   blocks one lane per block: its file by an upper-bound binary search of
//          first[] (at most 32 steps on an array that stays in L2), its
//          FILE_BLOCK at block_at(i), byte stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sf_device.hpp"
#include "sf_wire_send_files.hpp"

namespace {

constexpr uint64_t kMaxMessages = 1ull << 32;
constexpr uint64_t kFilesMaxPerLaunch = 1ull << 30;  // lanes per launch (grid x stays far below 2^31)

// The smallest k among the wave's lanes with `bad`, to *first (which starts
// at UINT64_MAX): one atomic per wave that has one.
__device__ __forceinline__ void first_bad(bool bad, uint64_t k, unsigned long long* first) {
  const unsigned long long m = __ballot(bad);
  if (m && (threadIdx.x & 63u) == (uint32_t)__ffsll(m) - 1) atomicMin(first, (unsigned long long)k);
}

// Files [base, base + n) of n_files.  back[0]: the FILE_BLOCK bytes, back[1]:
// the name bytes (both from the last file's lane), back[2]: the first bad file.
__global__ void __launch_bounds__(256) files_check_kernel(const uint64_t* __restrict__ first,
                                                          const uint8_t* __restrict__ names,
                                                          const uint64_t* __restrict__ name_at, uint64_t n_files,
                                                          uint64_t n_blocks, const uint64_t* __restrict__ ends,
                                                          uint64_t base, uint64_t n,
                                                          unsigned long long* __restrict__ back) {
  const uint64_t f = base + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = f < base + n;
  first_bad(in && !sfwp::file_ok(first, names, name_at, n_files, n_blocks, f), f, back + 2);
  if (in && f + 1 == n_files) {
    back[0] = sfwp::bex(ends, n_blocks);
    back[1] = name_at[n_files];
  }
}

__global__ void __launch_bounds__(256) files_frames_kernel(const uint64_t* __restrict__ first,
                                                           const uint8_t* __restrict__ names,
                                                           const uint64_t* __restrict__ name_at,
                                                           const uint64_t* __restrict__ ends, uint64_t base,
                                                           uint64_t n, uint8_t* __restrict__ out) {
  const uint64_t f = base + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= base + n) return;
  const uint64_t a0 = name_at[f];
  sfwp::write_file_start(out + sfwp::start_at(ends, first, name_at, f), names + a0, (uint32_t)(name_at[f + 1] - a0));
  sfwp::write_file_end(out + sfwp::end_at(ends, first, name_at, f));
}

__global__ void __launch_bounds__(256) files_blocks_kernel(const uint8_t* __restrict__ digests,
                                                           const uint32_t* __restrict__ sizes,
                                                           const uint64_t* __restrict__ first,
                                                           const uint64_t* __restrict__ name_at, uint64_t n_files,
                                                           const uint64_t* __restrict__ ends, uint64_t base,
                                                           uint64_t n, uint8_t* __restrict__ out) {
  const uint64_t i = base + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= base + n) return;
  const uint64_t f = sfwp::file_of_block(first, n_files, i);
  sfwp::write_file_block(out + sfwp::block_at(ends, name_at, f, i), digests + sfwp::kDigest * i, sizes[i]);
}

}  // namespace

using namespace sfi;

namespace {

int wire_files(const uint8_t* d_digests, const uint32_t* d_sizes, uint64_t n_blocks, const uint64_t* d_first,
               const uint8_t* d_names, const uint64_t* d_name_at, uint64_t n_files, sf_wire_run** out,
               uint64_t* bad_file, hipStream_t s) {
  if (out) *out = nullptr;
  if (bad_file) *bad_file = UINT64_MAX;
  if (!out || !bad_file) return SF_EINVAL;
  if (misaligned(d_digests, 4) || misaligned(d_sizes, 4) || misaligned(d_first, 8) || misaligned(d_name_at, 8))
    return SF_EINVAL;
  if (n_blocks > kMaxMessages || n_files > kMaxMessages / 2 || n_blocks + 2 * n_files > kMaxMessages) return SF_EINVAL;
  if (n_files == 0) {
    if (n_blocks) return SF_EINVAL;  // blocks of no file
    *out = wire_run_empty();
    return SF_OK;
  }
  if (!d_first || !d_name_at || (n_blocks && (!d_digests || !d_sizes))) return SF_EINVAL;

  Scratch plan(s);  // wire_plan's allocation: E first
  if (n_blocks) {
    uint64_t* e = nullptr;
    const int rc = wire_plan(d_sizes, n_blocks, &e, s);
    if (rc != SF_OK) return rc;
    plan.p = e;
  }
  const uint64_t* ends = static_cast<const uint64_t*>(plan.p);
  ScratchLayout L;
  const size_t back_at = L.add(24);  // the three words that come back
  Scratch ws(s);
  int rc = stream_alloc(&ws.p, L.total(), s);
  if (rc != SF_OK) return rc;
  unsigned long long* d_back = L.at<unsigned long long>(ws.p, back_at);
  SF_HIP(hipMemsetAsync(d_back, 0xFF, 24, s));
  rc = for_pieces(n_files, kFilesMaxPerLaunch, [&](uint64_t base, uint64_t cnt) {
    return launch(files_check_kernel, grid256(cnt), dim3(256), s, d_first, d_names, d_name_at, n_files, n_blocks, ends,
                  base, cnt, d_back);
  });
  if (rc != SF_OK) return rc;
  uint64_t back[3] = {0, 0, 0};  // FILE_BLOCK bytes, name bytes, the first bad file
  SF_HIP(hipMemcpyAsync(back, d_back, 24, hipMemcpyDeviceToHost, s));
  SF_HIP(hipStreamSynchronize(s));
  if (back[2] != UINT64_MAX) {
    *bad_file = back[2];
    return SF_EINVAL;
  }
  const uint64_t total = sfwp::files_run_total(back[0], back[1], n_files);

  sf_wire_run* run = nullptr;
  rc = wire_run_begin(total, n_blocks + 2 * n_files, s, &run);
  if (rc == SF_OK)
    rc = for_pieces(n_files, kFilesMaxPerLaunch, [&](uint64_t base, uint64_t cnt) {
      return launch(files_frames_kernel, grid256(cnt), dim3(256), s, d_first, d_names, d_name_at, ends, base, cnt,
                    run->bytes);
    });
  if (rc == SF_OK)
    rc = for_pieces(n_blocks, kFilesMaxPerLaunch, [&](uint64_t base, uint64_t cnt) {
      return launch(files_blocks_kernel, grid256(cnt), dim3(256), s, d_digests, d_sizes, d_first, d_name_at, n_files,
                    ends, base, cnt, run->bytes);
    });
  return wire_run_finish(run, rc, s, out);
}

}  // namespace

extern "C" int sf_wire_files_device(const void* d_digests, const uint32_t* d_sizes, uint64_t n_blocks,
                                    const uint64_t* d_file_first, const void* d_names, const uint64_t* d_name_at,
                                    uint64_t n_files, sf_wire_run** run, uint64_t* bad_file, void* stream) {
  return guarded([&] {
    return wire_files(static_cast<const uint8_t*>(d_digests), d_sizes, n_blocks, d_file_first,
                      static_cast<const uint8_t*>(d_names), d_name_at, n_files, run, bad_file, as_stream(stream));
  });
}
