// sf_want.hip -- the destination's missing blocks on the device (include/
// syncfast_amd.h: sf_wire_get_blocks_device, sf_place_block_data_device).
// After the FILE_BLOCK runs the reference's sink lists the rows with
// present = 0 and writes one GET_BLOCK per row (src/sync/fs.rs:485-493,
// src/sync/ssh/proto.rs:170-174); for every BLOCK_DATA that comes back it asks
// the index where that hash is wanted and writes the payload there, one query
// and one update per message (fs.rs:505-510).  Here the missing-row list stays
// in HBM: its request run is built there, and a parsed BLOCK_DATA run is joined
// against it there, into the three lists sf_copy_blocks_device takes.
// Its own translation unit: the other kernels' code objects stay as they are.
// The per-row rules are sf_want_plan.hpp's, shared with the host test that
// executes them.  Random-access, latency-bound integer work: no MFMA, no LDS.
//
// Every dependency is a kernel boundary (no lane waits for another wave), and
// atomics go on counters only:
//
//   requests  ask      one lane per row: the byte flag "this row asks".
//             distinct sf_block_set_build over the asking rows, a lookup of
//                      every row's own digest, and a row keeps its flag when
//                      the answer is itself (the set keeps the smallest row).
//             scan     rocprim inclusive scan of the flags, uint64; the last
//                      entry comes back: the call's only read-back.
//             emit     one lane per row: an asking row writes its 31 bytes at
//                      31 (scan - 1), byte stores (the run is not aligned to
//                      anything a row could use: 31 is odd).
//   join      lookup   sf_block_set_build over the ok messages, a lookup of
//                      the row digests: the lowest-numbered ok message per row.
//             class    one lane per row: nothing, a job, or a size mismatch;
//                      the waiting rows and the mismatches are counted, one
//                      atomic per wave that has any.
//             scan     of "is a job", uint64; the job count and the two
//                      counters come back in one 24-byte copy.  Nothing has
//                      been marked or written up to here.
//             emit     one lane per row: a job row writes entry scan - 1 of
//                      the five lists, marks itself present and counts its
//                      message's use (an atomic on that message's counter).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/iterator/transform_iterator.hpp>

#include "sf_device.hpp"
#include "sf_want_plan.hpp"

namespace {

constexpr uint64_t kMaxRows = 1ull << 31;  // one lane per row, one launch: the grid's x stays below 2^23

struct IsSet {
  __host__ __device__ uint64_t operator()(uint8_t f) const { return f == 1 ? 1ull : 0ull; }
};

// The wave's lanes with `on`, added to *counter by one lane when there are
// any.  Every lane of the wave calls it.
__device__ __forceinline__ void count_wave(bool on, unsigned long long* counter) {
  const unsigned long long m = __ballot(on);
  if (m && (threadIdx.x & 63u) == 0) atomicAdd(counter, (unsigned long long)__popcll(m));
}

__global__ void __launch_bounds__(256) want_ask_kernel(const int64_t* __restrict__ rows,
                                                       const uint8_t* __restrict__ take, uint64_t n,
                                                       uint8_t* __restrict__ ask) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) ask[i] = sfwt::asks(rows, take, i) ? 1 : 0;
}

// found[i]: the first asking row with row i's digest (an asking row finds at
// least itself).
__global__ void __launch_bounds__(256) want_first_kernel(const int64_t* __restrict__ found, uint64_t n,
                                                         uint8_t* __restrict__ ask) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && ask[i] && found[i] != (int64_t)i) ask[i] = 0;
}

__global__ void __launch_bounds__(256) want_emit_kernel(const uint8_t* __restrict__ digests,
                                                        const uint8_t* __restrict__ ask,
                                                        const uint64_t* __restrict__ ends, uint64_t n,
                                                        uint8_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !ask[i]) return;
  const uint32_t* p = reinterpret_cast<const uint32_t*>(digests + i * sfwp::kDigest);  // rows are 4-B aligned
  uint8_t d[sfwp::kDigest];
#pragma unroll
  for (uint32_t w = 0; w < 5; w++) {
    const uint32_t v = p[w];
    d[4 * w] = (uint8_t)v, d[4 * w + 1] = (uint8_t)(v >> 8), d[4 * w + 2] = (uint8_t)(v >> 16),
          d[4 * w + 3] = (uint8_t)(v >> 24);
  }
  sfwt::write_get_block(out + sfwp::kGetBlock * (ends[i] - 1), d);
}

// cls[r] = what becomes of row r (sfwt::Place); counters[0] += the rows that
// wait, counters[1] += the size mismatches.  found NULL: no message at all.
__global__ void __launch_bounds__(256) place_class_kernel(const uint8_t* __restrict__ present,
                                                          const uint32_t* __restrict__ row_sizes,
                                                          const int64_t* __restrict__ found,
                                                          const uint32_t* __restrict__ msg_sizes, uint64_t n,
                                                          uint8_t* __restrict__ cls,
                                                          unsigned long long* __restrict__ counters) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = r < n;
  const uint8_t here = in ? present[r] : 1;
  int c = sfwt::kNone;
  if (here == 0 && found) {
    const int64_t m = found[r];
    c = sfwt::place(here, m, m >= 0 ? msg_sizes[m] : 0, row_sizes[r]);
  }
  if (in) cls[r] = (uint8_t)c;
  count_wave(here == 0, counters);
  count_wave(c == sfwt::kMismatch, counters + 1);
}

__global__ void __launch_bounds__(256) place_emit_kernel(
    const uint8_t* __restrict__ cls, const uint64_t* __restrict__ ends, const int64_t* __restrict__ found,
    const uint32_t* __restrict__ row_sizes, const uint64_t* __restrict__ row_dst,
    const uint64_t* __restrict__ msg_off, uint64_t n, uint8_t* __restrict__ present, uint64_t* __restrict__ src_off,
    uint64_t* __restrict__ dst_off, uint32_t* __restrict__ sizes, int64_t* __restrict__ job_rows,
    int64_t* __restrict__ job_msgs, uint32_t* __restrict__ uses) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n || cls[r] != sfwt::kJob) return;
  const uint64_t k = ends[r] - 1;
  const int64_t m = found[r];
  src_off[k] = msg_off[m];
  dst_off[k] = row_dst[r];
  sizes[k] = row_sizes[r];
  job_rows[k] = (int64_t)r;
  job_msgs[k] = m;
  present[r] = 1;
  if (uses) atomicAdd(&uses[m], 1u);
}

}  // namespace

using namespace sfi;

namespace {

// A block set that is given back on every path out of a call.
struct Set {
  sf_block_set* p = nullptr;
  hipStream_t s;
  explicit Set(hipStream_t s_) : s(s_) {}
  ~Set() { (void)sf_block_set_free(p, s); }
  Set(const Set&) = delete;
  Set& operator=(const Set&) = delete;
};

using Flags = rocprim::transform_iterator<const uint8_t*, IsSet, uint64_t>;

// ends[i] = the flags that are 1 in flags[0 .. i]; tmp NULL: the temporary's size alone
int scan_flags(void* tmp, size_t& tmp_bytes, const uint8_t* flags, uint64_t* ends, uint64_t n, hipStream_t s) {
  return scan_inclusive(tmp, tmp_bytes, Flags(flags, IsSet()), ends, n, s);
}

int get_blocks(const uint8_t* d_digests, const int64_t* d_rows, const uint8_t* d_take, uint64_t n, int distinct,
               sf_wire_run** out, uint64_t* n_requests, hipStream_t s) {
  if (!out) return SF_EINVAL;
  *out = nullptr;
  if (n_requests) *n_requests = 0;
  if (n > kMaxRows || misaligned(d_rows, 8)) return SF_EINVAL;
  if (n && (!d_digests || misaligned(d_digests, 4))) return SF_EINVAL;
  if (n == 0) {
    *out = wire_run_empty();
    return SF_OK;
  }
  size_t tmp = 0;
  int rc = scan_flags(nullptr, tmp, nullptr, nullptr, n, s);
  if (rc != SF_OK) return rc;
  // the scan's end offsets, the lookup's rows (distinct), the flags, the scan's
  ScratchLayout L;
  const size_t ends_at = L.add(n * 8), found_at = L.add(distinct ? n * 8 : 0), ask_at = L.add(n);
  Scratch ws(s);
  rc = stream_alloc(&ws.p, L.total() + tmp + 8, s);
  if (rc != SF_OK) return rc;
  uint64_t* ends = L.at<uint64_t>(ws.p, ends_at);
  int64_t* found = L.at<int64_t>(ws.p, found_at);
  uint8_t* ask = L.at<uint8_t>(ws.p, ask_at);
  void* scan_tmp = L.at<void>(ws.p, L.total());

  rc = launch(want_ask_kernel, grid256(n), dim3(256), s, d_rows, d_take, n, ask);
  if (rc != SF_OK) return rc;
  if (distinct) {
    Set set(s);
    rc = sf_block_set_build(d_digests, ask, n, &set.p, s);
    if (rc == SF_OK) rc = sf_block_set_lookup(set.p, d_digests, n, found, s);
    if (rc == SF_OK) rc = launch(want_first_kernel, grid256(n), dim3(256), s, found, n, ask);
    if (rc != SF_OK) return rc;
  }
  rc = scan_flags(scan_tmp, tmp, ask, ends, n, s);
  if (rc != SF_OK) return rc;
  uint64_t count = 0;
  SF_HIP(hipMemcpyAsync(&count, ends + n - 1, 8, hipMemcpyDeviceToHost, s));
  SF_HIP(hipStreamSynchronize(s));
  if (count == 0) {
    *out = wire_run_empty();
    return SF_OK;
  }

  sf_wire_run* run = nullptr;
  rc = wire_run_begin(count * sfwp::kGetBlock, count, s, &run);
  if (rc == SF_OK) rc = launch(want_emit_kernel, grid256(n), dim3(256), s, d_digests, ask, ends, n, run->bytes);
  rc = wire_run_finish(run, rc, s, out);
  if (rc == SF_OK && n_requests) *n_requests = count;
  return rc;
}

int place_block_data(const uint8_t* d_row_digests, const uint32_t* d_row_sizes, const uint64_t* d_row_dst,
                     uint8_t* d_row_present, uint64_t n_rows, const uint8_t* d_msg_digests,
                     const uint32_t* d_msg_sizes, const uint64_t* d_msg_off, const uint8_t* d_msg_ok, uint64_t n_msgs,
                     uint64_t* d_src_off, uint64_t* d_dst_off, uint32_t* d_sizes, int64_t* d_job_rows,
                     int64_t* d_job_msgs, uint64_t cap, uint32_t* d_msg_uses, uint64_t* n_jobs, uint64_t* n_left,
                     uint64_t* n_size_mismatch, hipStream_t s) {
  if (!n_jobs || !n_left || !n_size_mismatch) return SF_EINVAL;
  *n_jobs = *n_left = *n_size_mismatch = 0;
  if (n_rows > kMaxRows || n_msgs > kMaxRows) return SF_EINVAL;
  if (n_rows && (!d_row_digests || !d_row_sizes || !d_row_dst || !d_row_present)) return SF_EINVAL;
  if (n_msgs && (!d_msg_digests || !d_msg_sizes || !d_msg_off)) return SF_EINVAL;
  if (misaligned(d_row_digests, 4) || misaligned(d_row_sizes, 4) || misaligned(d_row_dst, 8) ||
      misaligned(d_msg_digests, 4) || misaligned(d_msg_sizes, 4) || misaligned(d_msg_off, 8) ||
      misaligned(d_src_off, 8) || misaligned(d_dst_off, 8) || misaligned(d_sizes, 4) || misaligned(d_job_rows, 8) ||
      misaligned(d_job_msgs, 8) || misaligned(d_msg_uses, 4))
    return SF_EINVAL;
  if (n_rows == 0) {  // no job: every message is unused
    if (d_msg_uses && n_msgs) SF_HIP(hipMemsetAsync(d_msg_uses, 0, n_msgs * 4, s));
    return SF_OK;
  }
  const bool have = n_msgs != 0;
  size_t tmp = 0;
  int rc = have ? scan_flags(nullptr, tmp, nullptr, nullptr, n_rows, s) : SF_OK;
  if (rc != SF_OK) return rc;
  // end offsets with the two counters behind them (read back together), the
  // lookup's messages, the rows' classes, the scan's
  ScratchLayout L;
  const size_t ends_at = L.add((n_rows + 2) * 8), found_at = L.add(n_rows * 8), cls_at = L.add(n_rows);
  Scratch ws(s);
  rc = stream_alloc(&ws.p, L.total() + tmp + 8, s);
  if (rc != SF_OK) return rc;
  uint64_t* ends = L.at<uint64_t>(ws.p, ends_at);
  unsigned long long* counters = reinterpret_cast<unsigned long long*>(ends + n_rows);
  int64_t* found = L.at<int64_t>(ws.p, found_at);
  uint8_t* cls = L.at<uint8_t>(ws.p, cls_at);
  void* scan_tmp = L.at<void>(ws.p, L.total());
  SF_HIP(hipMemsetAsync(counters, 0, 16, s));
  if (have) {
    Set set(s);
    rc = sf_block_set_build(d_msg_digests, d_msg_ok, n_msgs, &set.p, s);
    if (rc == SF_OK) rc = sf_block_set_lookup(set.p, d_row_digests, n_rows, found, s);
    if (rc != SF_OK) return rc;
  }
  rc = launch(place_class_kernel, grid256(n_rows), dim3(256), s, d_row_present, d_row_sizes, have ? found : nullptr,
              d_msg_sizes, n_rows, cls, counters);
  if (rc != SF_OK) return rc;
  uint64_t back[3] = {0, 0, 0};  // the jobs, the rows that wait, the size mismatches
  if (have) {
    rc = scan_flags(scan_tmp, tmp, cls, ends, n_rows, s);
    if (rc != SF_OK) return rc;
    SF_HIP(hipMemcpyAsync(back, ends + n_rows - 1, 24, hipMemcpyDeviceToHost, s));
  } else {
    SF_HIP(hipMemcpyAsync(back + 1, counters, 16, hipMemcpyDeviceToHost, s));
  }
  SF_HIP(hipStreamSynchronize(s));
  const uint64_t jobs = back[0];
  *n_jobs = jobs;
  *n_size_mismatch = back[2];
  if (jobs && (jobs > cap || !d_src_off || !d_dst_off || !d_sizes || !d_job_rows || !d_job_msgs)) {
    *n_left = back[1];  // nothing was marked
    return SF_ENOSPC;
  }
  *n_left = back[1] - jobs;
  if (d_msg_uses && n_msgs) SF_HIP(hipMemsetAsync(d_msg_uses, 0, n_msgs * 4, s));
  if (!jobs) return SF_OK;
  return launch(place_emit_kernel, grid256(n_rows), dim3(256), s, cls, ends, found, d_row_sizes, d_row_dst, d_msg_off,
                n_rows, d_row_present, d_src_off, d_dst_off, d_sizes, d_job_rows, d_job_msgs, d_msg_uses);
}

}  // namespace

extern "C" {

int sf_wire_get_blocks_device(const void* d_digests, const int64_t* d_rows, const uint8_t* d_take, uint64_t n_rows,
                              int distinct, sf_wire_run** out, uint64_t* n_requests, void* stream) {
  return guarded([&] {
    return get_blocks(static_cast<const uint8_t*>(d_digests), d_rows, d_take, n_rows, distinct, out, n_requests,
                      as_stream(stream));
  });
}

int sf_place_block_data_device(const void* d_row_digests, const uint32_t* d_row_sizes, const uint64_t* d_row_dst,
                               uint8_t* d_row_present, uint64_t n_rows, const void* d_msg_digests,
                               const uint32_t* d_msg_sizes, const uint64_t* d_msg_data_offsets,
                               const uint8_t* d_msg_ok, uint64_t n_msgs, uint64_t* d_src_offsets,
                               uint64_t* d_dst_offsets, uint32_t* d_sizes, int64_t* d_job_rows, int64_t* d_job_msgs,
                               uint64_t cap, uint32_t* d_msg_uses, uint64_t* n_jobs, uint64_t* n_left,
                               uint64_t* n_size_mismatch, void* stream) {
  return guarded([&] {
    return place_block_data(static_cast<const uint8_t*>(d_row_digests), d_row_sizes, d_row_dst, d_row_present, n_rows,
                            static_cast<const uint8_t*>(d_msg_digests), d_msg_sizes, d_msg_data_offsets, d_msg_ok,
                            n_msgs, d_src_offsets, d_dst_offsets, d_sizes, d_job_rows, d_job_msgs, cap, d_msg_uses,
                            n_jobs, n_left, n_size_mismatch, as_stream(stream));
  });
}

}  // extern "C"
