// sf_send_entries.hip -- the two runs of the files-list phase built on the
// device (include/syncfast_amd.h): the source's list, one FILE_ENTRY per file
// and END_FILES (sf_wire_file_entries_device; FsSource's ListFiles state,
// src/sync/fs.rs:133-164, written by write_message, src/sync/ssh/proto.rs:
// 142-151), and the destination's GET_FILE requests for the entries it needs
// (sf_wire_get_files_device; fs.rs:415-443, proto.rs:152-156).  The receiving
// half of the list is sf_recv_entries.hip.  Its own translation unit: the other
// kernels' code objects stay as they are.  The messages' lengths, their
// writers and the per-message tests are sf_wire_entries.hpp's, shared with the
// host test that executes them.
//
// Both runs go the same way, ordered by kernel boundaries only (no lane waits
// for another wave):
//
//   lengths  one lane per message: entry_ok / pick_ok of what it is made from
//            (the smallest failing one is an atomicMin, one per wave) and the
//            message's length, 0 for one that fails.
//   scan     rocprim inclusive scan of the lengths in 64 bits: where every
//            message ends.
//   (one read-back: the first bad message and the scan's last entry; the run
//    is allocated then)
//   write    one lane per message writes it at its place with byte stores; one
//            more lane writes END_FILES.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sf_device.hpp"
#include "sf_wire_entries.hpp"

namespace {

constexpr uint64_t kMaxEntries = 1ull << 31;  // messages per call: one launch, one lane each

// The smallest k among the wave's lanes with `bad`, to *first (which starts
// at UINT64_MAX): one atomic per wave that has one.
__device__ __forceinline__ void first_bad(bool bad, uint64_t k, unsigned long long* first) {
  const unsigned long long m = __ballot(bad);
  if (m && (threadIdx.x & 63u) == (uint32_t)__ffsll(m) - 1) atomicMin(first, (unsigned long long)k);
}

__global__ void __launch_bounds__(256) entries_lengths_kernel(const uint8_t* __restrict__ names,
                                                              const uint64_t* __restrict__ name_at,
                                                              const uint64_t* __restrict__ sizes, uint64_t n,
                                                              uint32_t* __restrict__ lens,
                                                              unsigned long long* __restrict__ bad) {
  const uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = f < n;
  const bool ok = in && sfwp::entry_ok(names, name_at, sizes, n, f);
  first_bad(in && !ok, f, bad);
  if (in) lens[f] = ok ? sfwp::file_entry_len((uint32_t)(name_at[f + 1] - name_at[f]), sizes[f]) : 0u;
}

// Lanes [0, n): the entries; lane n: END_FILES behind them, when asked for.
__global__ void __launch_bounds__(256) entries_write_kernel(const uint8_t* __restrict__ names,
                                                            const uint64_t* __restrict__ name_at,
                                                            const uint64_t* __restrict__ sizes,
                                                            const uint8_t* __restrict__ hashes, uint64_t n,
                                                            const uint32_t* __restrict__ lens,
                                                            const uint64_t* __restrict__ ends, int end_files,
                                                            uint8_t* __restrict__ out) {
  const uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f < n) {
    const uint64_t a0 = name_at[f];
    sfwp::write_file_entry(out + (ends[f] - lens[f]), names + a0, (uint32_t)(name_at[f + 1] - a0), sizes[f],
                           hashes + sfwp::kDigest * f);
  } else if (f == n && end_files) {
    sfwp::write_end_files(out + (n ? ends[n - 1] : 0));
  }
}

__global__ void __launch_bounds__(256) get_files_lengths_kernel(const uint8_t* __restrict__ bytes, uint64_t n_bytes,
                                                                const uint64_t* __restrict__ at,
                                                                const uint32_t* __restrict__ len, uint64_t n,
                                                                const uint32_t* __restrict__ pick, uint64_t n_pick,
                                                                uint32_t* __restrict__ lens,
                                                                unsigned long long* __restrict__ bad) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = k < n_pick;
  uint64_t i = 0;
  const bool ok = in && sfwp::pick_ok(bytes, n_bytes, at, len, n, pick, k, &i);
  first_bad(in && !ok, k, bad);
  if (in) lens[k] = ok ? sfwp::get_file_len(len[i]) : 0u;
}

__global__ void __launch_bounds__(256) get_files_write_kernel(const uint8_t* __restrict__ bytes,
                                                              const uint64_t* __restrict__ at,
                                                              const uint32_t* __restrict__ len,
                                                              const uint32_t* __restrict__ pick, uint64_t n_pick,
                                                              const uint32_t* __restrict__ lens,
                                                              const uint64_t* __restrict__ ends,
                                                              uint8_t* __restrict__ out) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_pick) return;
  const uint64_t i = pick ? pick[k] : k;
  sfwp::write_get_file(out + (ends[k] - lens[k]), bytes + at[i], len[i]);
}

}  // namespace

using namespace sfi;

namespace {

// What both runs share: the lengths of m messages (m > 0) are written by
// `lengths(lens, bad)` and scanned; *total = the scan's last entry and *bad =
// the first failing message come back in one synchronisation.  ws keeps lens
// and ends for the write kernel.
template <typename F>
int plan_messages(uint64_t m, hipStream_t s, Scratch& ws, uint32_t** lens, uint64_t** ends, uint64_t* total,
                  uint64_t* bad, F&& lengths) {
  size_t tmp = 0;
  int rc = scan_inclusive(nullptr, tmp, static_cast<uint32_t*>(nullptr), static_cast<uint64_t*>(nullptr), m, s);
  if (rc != SF_OK) return rc;
  ScratchLayout L;
  const size_t bad_at = L.add(8), ends_at = L.add(m * 8), lens_at = L.add(m * 4);
  if ((rc = stream_alloc(&ws.p, L.total() + tmp + 8, s)) != SF_OK) return rc;
  unsigned long long* d_bad = L.at<unsigned long long>(ws.p, bad_at);
  *lens = L.at<uint32_t>(ws.p, lens_at);
  *ends = L.at<uint64_t>(ws.p, ends_at);
  SF_HIP(hipMemsetAsync(d_bad, 0xFF, 8, s));
  if ((rc = lengths(*lens, d_bad)) != SF_OK) return rc;
  if ((rc = scan_inclusive(L.at<void>(ws.p, L.total()), tmp, *lens, *ends, m, s)) != SF_OK) return rc;
  SF_HIP(hipMemcpyAsync(bad, d_bad, 8, hipMemcpyDeviceToHost, s));
  SF_HIP(hipMemcpyAsync(total, *ends + (m - 1), 8, hipMemcpyDeviceToHost, s));
  SF_HIP(hipStreamSynchronize(s));
  return SF_OK;
}

int wire_file_entries(const uint8_t* d_names, const uint64_t* d_name_at, const uint64_t* d_sizes,
                      const uint8_t* d_hashes, uint64_t n, int end_files, sf_wire_run** out, uint64_t* bad_file,
                      hipStream_t s) {
  if (out) *out = nullptr;
  if (bad_file) *bad_file = UINT64_MAX;
  if (!out || !bad_file || n > kMaxEntries) return SF_EINVAL;
  if (misaligned(d_name_at, 8) || misaligned(d_sizes, 8) || misaligned(d_hashes, 4)) return SF_EINVAL;
  if (n && (!d_name_at || !d_sizes || !d_hashes)) return SF_EINVAL;
  if (n == 0 && !end_files) {
    *out = wire_run_empty();
    return SF_OK;
  }
  Scratch ws(s);
  uint32_t* lens = nullptr;
  uint64_t* ends = nullptr;
  uint64_t total = 0, bad = UINT64_MAX;
  if (n) {
    const int rc = plan_messages(n, s, ws, &lens, &ends, &total, &bad, [&](uint32_t* l, unsigned long long* b) {
      return launch(entries_lengths_kernel, grid256(n), dim3(256), s, d_names, d_name_at, d_sizes, n, l, b);
    });
    if (rc != SF_OK) return rc;
    if (bad != UINT64_MAX) {
      *bad_file = bad;
      return SF_EINVAL;
    }
  }
  sf_wire_run* run = nullptr;
  int rc = wire_run_begin(total + (end_files ? sfwp::kEndFilesTag : 0), n + (end_files ? 1 : 0), s, &run);
  if (rc == SF_OK)
    rc = launch(entries_write_kernel, grid256(n + 1), dim3(256), s, d_names, d_name_at, d_sizes, d_hashes, n, lens,
                ends, end_files, run->bytes);
  return wire_run_finish(run, rc, s, out);
}

int wire_get_files(const uint8_t* d_bytes, uint64_t n_bytes, const uint64_t* d_name_at, const uint32_t* d_name_len,
                   uint64_t n, const uint32_t* d_pick, uint64_t n_pick, sf_wire_run** out, uint64_t* bad_pick,
                   hipStream_t s) {
  if (out) *out = nullptr;
  if (bad_pick) *bad_pick = UINT64_MAX;
  if (!out || !bad_pick) return SF_EINVAL;
  if (!d_pick) n_pick = n;
  if (n > kMaxEntries || n_pick > kMaxEntries) return SF_EINVAL;
  if (misaligned(d_name_at, 8) || misaligned(d_name_len, 4) || misaligned(d_pick, 4)) return SF_EINVAL;
  if ((n && (!d_name_at || !d_name_len)) || (n_bytes && !d_bytes)) return SF_EINVAL;
  if (n_pick == 0) {
    *out = wire_run_empty();
    return SF_OK;
  }
  Scratch ws(s);
  uint32_t* lens = nullptr;
  uint64_t* ends = nullptr;
  uint64_t total = 0, bad = UINT64_MAX;
  int rc = plan_messages(n_pick, s, ws, &lens, &ends, &total, &bad, [&](uint32_t* l, unsigned long long* b) {
    return launch(get_files_lengths_kernel, grid256(n_pick), dim3(256), s, d_bytes, n_bytes, d_name_at, d_name_len, n,
                  d_pick, n_pick, l, b);
  });
  if (rc != SF_OK) return rc;
  if (bad != UINT64_MAX) {
    *bad_pick = bad;
    return SF_EINVAL;
  }
  sf_wire_run* run = nullptr;
  rc = wire_run_begin(total, n_pick, s, &run);
  if (rc == SF_OK)
    rc = launch(get_files_write_kernel, grid256(n_pick), dim3(256), s, d_bytes, d_name_at, d_name_len, d_pick, n_pick,
                lens, ends, run->bytes);
  return wire_run_finish(run, rc, s, out);
}

}  // namespace

extern "C" {

int sf_wire_file_entries_device(const void* d_names, const uint64_t* d_name_at, const uint64_t* d_sizes,
                                const void* d_hashes, uint64_t n_files, int end_files, sf_wire_run** run,
                                uint64_t* bad_file, void* stream) {
  return guarded([&] {
    return wire_file_entries(static_cast<const uint8_t*>(d_names), d_name_at, d_sizes,
                             static_cast<const uint8_t*>(d_hashes), n_files, end_files, run, bad_file,
                             as_stream(stream));
  });
}

int sf_wire_get_files_device(const void* d_bytes, uint64_t n_bytes, const uint64_t* d_name_at,
                             const uint32_t* d_name_len, uint64_t n, const uint32_t* d_pick, uint64_t n_pick,
                             sf_wire_run** run, uint64_t* bad, void* stream) {
  return guarded([&] {
    return wire_get_files(static_cast<const uint8_t*>(d_bytes), n_bytes, d_name_at, d_name_len, n, d_pick, n_pick, run,
                          bad, as_stream(stream));
  });
}

}  // extern "C"
