// sf_send.hip -- the sending side of the block exchange (include/
// syncfast_amd.h: sf_wire_block_data_device, sf_serve_get_blocks_device and
// the run handle).  The reference's source answers every GET_BLOCK with a
// BLOCK_DATA message: Index::get_block, read_block, write_message
// (src/sync/fs.rs:199-208, src/sync/ssh/proto.rs:175-181), one block at a
// time.  Here a whole request run is answered in one call, from HBM to HBM.
// Its own translation unit: the other kernels' code objects stay as they are.
// The framing rules are sf_wire_data.hpp's, shared with the host test that
// executes them.
//
// A run of n jobs, ordered by kernel boundaries only (no lane waits for
// another wave):
//
//   plan     one lane per job: the message's length 34 + digits(size) + size
//            to lens[i]; a job whose source leaves [0, src_len) sets a flag.
//   scan     rocprim inclusive scan of the lengths into end offsets, uint64.
//            The last end offset and the flag come back in one 16-byte copy:
//            the call's only read-back.  The run is allocated then.
//   headers  one lane per message, byte stores: the header at ends[i] -
//            lens' value, the end byte at ends[i] - 1, and the payload's
//            offset ends[i] - 1 - size to a scratch list.  No store touches a
//            payload byte.
//   payloads sfi::copy_blocks (sf_copy.hip) with the caller's source offsets
//            and that list: byte stores at a payload's edges, aligned 16-byte
//            stores between, none outside its range -- so the headers written
//            before it on the stream stay as they are.
//
// A request run: one lane per 31-byte slot tests the tag line and the end
// byte, and the first slot that fails is an atomicMin (one per wave); the
// digests before it are gathered into a 4-byte aligned table and looked up in
// the block set; one more kernel finds the first request without a row and
// turns the rows into a job list.  What stops the run is decided on the host
// by the serial rule, from the at most 128 bytes copied back from there.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sf_copy_plan.hpp"
#include "sf_device.hpp"
#include "sf_wire_data.hpp"

namespace {

constexpr uint64_t kMaxJobs = 1ull << 32;
constexpr uint64_t kMaxRequestBytes = 1ull << 38;
constexpr uint64_t kSendMaxPerLaunch = 1ull << 30;  // lanes per launch (grid x stays far below 2^31)
constexpr uint32_t kStopBytes = 128;                // copied back from where a request run stops

// The smallest k among the wave's lanes with `bad`, to *first (which starts
// at UINT64_MAX): one atomic per wave that has one.
__device__ __forceinline__ void first_bad(bool bad, uint64_t k, unsigned long long* first) {
  const unsigned long long m = __ballot(bad);
  if (m && (threadIdx.x & 63u) == (uint32_t)__ffsll(m) - 1) atomicMin(first, (unsigned long long)k);
}

__global__ void __launch_bounds__(256) send_plan_kernel(const uint64_t* __restrict__ src_off,
                                                        const uint32_t* __restrict__ sizes, uint64_t n,
                                                        uint64_t src_len, uint64_t* __restrict__ lens,
                                                        unsigned long long* __restrict__ flag) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t size = sizes[i];
  lens[i] = sfwp::block_data_len(size);
  if (!sfcp::in_range(src_off[i], size, src_len)) *flag = 1;  // every lane stores the same value
}

// Message i of messages [0, n) whose end offsets are ends[0, n): everything
// but its payload, and where its payload goes.
__global__ void __launch_bounds__(256) send_headers_kernel(const uint8_t* __restrict__ digests,
                                                           const uint32_t* __restrict__ sizes,
                                                           const uint64_t* __restrict__ ends, uint64_t n,
                                                           uint8_t* __restrict__ out,
                                                           uint64_t* __restrict__ dst_off) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t size = sizes[i];
  const uint64_t end = ends[i];
  sfwp::write_block_data(out + (end - sfwp::block_data_len(size)), out + (end - 1), digests + i * sfwp::kDigest, size);
  dst_off[i] = end - 1 - size;
}

__global__ void __launch_bounds__(256) send_slots_kernel(const uint8_t* __restrict__ req, uint64_t first, uint64_t n,
                                                         unsigned long long* __restrict__ first_fail) {
  const uint64_t k = first + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = k < first + n;
  first_bad(in && !sfwp::is_get_block(req + sfwp::kGetBlock * k), k, first_fail);
}

// Digest k of the requests [0, n) to the table's row k (dword stores: the
// table is 4-byte aligned, the run is not).
__global__ void __launch_bounds__(256) send_digests_kernel(const uint8_t* __restrict__ req, uint64_t first,
                                                           uint64_t n, uint32_t* __restrict__ table) {
  const uint64_t k = first + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= first + n) return;
  const uint8_t* d = req + sfwp::kGetBlock * k + sfwp::kGetTag;
#pragma unroll
  for (uint32_t w = 0; w < 5; w++)
    table[5 * k + w] = (uint32_t)d[4 * w] | (uint32_t)d[4 * w + 1] << 8 | (uint32_t)d[4 * w + 2] << 16 |
                       (uint32_t)d[4 * w + 3] << 24;
}

// Request k's job from its row: the row's block, or nothing and a candidate
// for the first request the set does not hold.
__global__ void __launch_bounds__(256) send_jobs_kernel(const int64_t* __restrict__ rows,
                                                        const uint64_t* __restrict__ row_off,
                                                        const uint32_t* __restrict__ row_size, uint64_t first,
                                                        uint64_t n, uint64_t* __restrict__ src_off,
                                                        uint32_t* __restrict__ sizes,
                                                        unsigned long long* __restrict__ first_missing) {
  const uint64_t k = first + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = k < first + n;
  const int64_t row = in ? rows[k] : 0;
  if (in) {
    src_off[k] = row >= 0 ? row_off[row] : 0;
    sizes[k] = row >= 0 ? row_size[row] : 0;
  }
  first_bad(in && row < 0, k, first_missing);
}

}  // namespace

using namespace sfi;

namespace {

void wire_run_discard(sf_wire_run* run, hipStream_t s) {
  stream_free(run->bytes, s);
  if (run->done) (void)hipEventDestroy(run->done);
  delete run;
}

}  // namespace

sf_wire_run* sfi::wire_run_empty() { return new sf_wire_run{nullptr, 0, 0, -1, nullptr}; }

int sfi::wire_run_begin(uint64_t n_bytes, uint64_t n_messages, hipStream_t s, sf_wire_run** out) {
  *out = nullptr;
  int dev = 0;
  SF_HIP(hipGetDevice(&dev));
  sf_wire_run* run = new sf_wire_run{nullptr, n_bytes, n_messages, dev, nullptr};
  int rc = stream_alloc(reinterpret_cast<void**>(&run->bytes), n_bytes, s);
  if (rc == SF_OK) rc = hip_err(hipEventCreateWithFlags(&run->done, hipEventDisableTiming));
  if (rc != SF_OK) {
    wire_run_discard(run, s);
    return rc;
  }
  *out = run;
  return SF_OK;
}

int sfi::wire_run_finish(sf_wire_run* run, int rc, hipStream_t s, sf_wire_run** out) {
  if (!run) return rc;
  if (rc == SF_OK) rc = hip_err(hipEventRecord(run->done, s));
  if (rc != SF_OK) {
    wire_run_discard(run, s);
    return rc;
  }
  *out = run;
  return SF_OK;
}

namespace {

int build_run(const uint8_t* d_src, uint64_t src_len, const uint8_t* d_digests, const uint64_t* d_src_off,
              const uint32_t* d_sizes, uint64_t n, sf_wire_run** out, hipStream_t s) {
  if (!out) return SF_EINVAL;
  *out = nullptr;
  if (n == 0) {
    *out = wire_run_empty();
    return SF_OK;
  }
  if (!d_src || !d_digests || !d_src_off || !d_sizes || n > kMaxJobs) return SF_EINVAL;
  if (misaligned(d_digests, 4) || misaligned(d_src_off, 8) || misaligned(d_sizes, 4)) return SF_EINVAL;
  // a job in range is at most 44 + src_len bytes of run: a list whose run
  // could pass 2^64 is not planned (the scan would wrap)
  uint64_t bound = 0;
  if (__builtin_mul_overflow(n, 44 + std::min<uint64_t>(src_len, 0xFFFFFFFFull), &bound)) return SF_ENOMEM;

  size_t tmp = 0;
  uint64_t* const nul = nullptr;
  int rc = scan_inclusive(nullptr, tmp, nul, nul, n, s);
  if (rc != SF_OK) return rc;
  // ends[0, n) and the flag behind them (read back together), lens, then the
  // payloads' offsets in the run, then the scan's
  ScratchLayout L;
  const size_t ends_at = L.add((n + 1) * 8), lens_at = L.add(n * 8), dst_at = L.add(n * 8);
  Scratch ws(s);
  rc = stream_alloc(&ws.p, L.total() + tmp + 8, s);
  if (rc != SF_OK) return rc;
  uint64_t* ends = L.at<uint64_t>(ws.p, ends_at);
  uint64_t* lens = L.at<uint64_t>(ws.p, lens_at);
  uint64_t* dst_off = L.at<uint64_t>(ws.p, dst_at);
  void* scan_tmp = L.at<void>(ws.p, L.total());
  unsigned long long* flag = reinterpret_cast<unsigned long long*>(ends + n);
  SF_HIP(hipMemsetAsync(flag, 0, 8, s));
  rc = for_pieces(n, kSendMaxPerLaunch, [&](uint64_t first, uint64_t cnt) {
    return launch(send_plan_kernel, grid256(cnt), dim3(256), s, d_src_off + first, d_sizes + first, cnt, src_len,
                  lens + first, flag);
  });
  if (rc == SF_OK) rc = scan_inclusive(scan_tmp, tmp, lens, ends, n, s);
  if (rc != SF_OK) return rc;
  uint64_t back[2] = {0, 0};  // the run's length, the flag
  SF_HIP(hipMemcpyAsync(back, ends + n - 1, 16, hipMemcpyDeviceToHost, s));
  SF_HIP(hipStreamSynchronize(s));
  if (back[1]) return SF_ERANGE;
  const uint64_t total = back[0];

  sf_wire_run* run = nullptr;
  rc = wire_run_begin(total, n, s, &run);
  if (rc == SF_OK)
    rc = for_pieces(n, kSendMaxPerLaunch, [&](uint64_t first, uint64_t cnt) {
      return launch(send_headers_kernel, grid256(cnt), dim3(256), s, d_digests + first * 20, d_sizes + first,
                    ends + first, cnt, run->bytes, dst_off + first);
    });
  if (rc == SF_OK) rc = copy_blocks(d_src, src_len, run->bytes, total, d_src_off, dst_off, d_sizes, nullptr, n, nullptr, s);
  return wire_run_finish(run, rc, s, out);
}

int serve(const sf_block_set* set, const uint64_t* d_row_off, const uint32_t* d_row_size, const uint8_t* d_src,
          uint64_t src_len, const uint8_t* d_req, uint64_t n_bytes, sf_wire_run** out, uint64_t* n_requests,
          uint64_t* n_answered, uint64_t* consumed, int* stop, hipStream_t s) {
  if (!out) return SF_EINVAL;
  *out = nullptr;
  if (!n_requests || !n_answered || !consumed || !stop) return SF_EINVAL;
  *n_requests = *n_answered = *consumed = 0;
  *stop = SF_WIRE_END;
  if (n_bytes > kMaxRequestBytes || (n_bytes && (!d_req || !set))) return SF_EINVAL;
  if (n_bytes == 0) {
    *out = wire_run_empty();
    return SF_OK;
  }
  const uint64_t slots = n_bytes / sfwp::kGetBlock;
  // first[0]: the first slot that is no message; first[1]: the first request
  // without a row (UINT64_MAX: none).  Then the digests, rows and jobs.
  ScratchLayout L;
  const size_t first_at = L.add(16), table_at = L.add(slots * 20), rows_at = L.add(slots * 8),
               src_at = L.add(slots * 8), sizes_at = L.add(slots * 4);
  Scratch ws(s);
  int rc = stream_alloc(&ws.p, L.total(), s);
  if (rc != SF_OK) return rc;
  unsigned long long* first = L.at<unsigned long long>(ws.p, first_at);
  uint32_t* table = L.at<uint32_t>(ws.p, table_at);
  int64_t* rows = L.at<int64_t>(ws.p, rows_at);
  uint64_t* src_off = L.at<uint64_t>(ws.p, src_at);
  uint32_t* sizes = L.at<uint32_t>(ws.p, sizes_at);
  SF_HIP(hipMemsetAsync(first, 0xFF, 16, s));
  rc = for_pieces(slots, kSendMaxPerLaunch, [&](uint64_t f, uint64_t cnt) {
    return launch(send_slots_kernel, grid256(cnt), dim3(256), s, d_req, f, cnt, first);
  });
  if (rc != SF_OK) return rc;
  uint64_t fail = 0;
  SF_HIP(hipMemcpyAsync(&fail, first, 8, hipMemcpyDeviceToHost, s));
  SF_HIP(hipStreamSynchronize(s));
  const uint64_t count = std::min(fail, slots), at = count * sfwp::kGetBlock;

  // what stands behind the messages, and which of them the set holds
  uint8_t tail[kStopBytes];
  const uint64_t avail = n_bytes - at, nt = std::min<uint64_t>(avail, kStopBytes);
  if (nt) SF_HIP(hipMemcpyAsync(tail, d_req + at, nt, hipMemcpyDeviceToHost, s));
  uint64_t missing = UINT64_MAX;
  if (count) {
    if (!d_row_off || !d_row_size) return SF_EINVAL;
    rc = for_pieces(count, kSendMaxPerLaunch, [&](uint64_t f, uint64_t cnt) {
      return launch(send_digests_kernel, grid256(cnt), dim3(256), s, d_req, f, cnt, table);
    });
    if (rc == SF_OK) rc = sf_block_set_lookup(set, table, count, rows, s);
    if (rc == SF_OK)
      rc = for_pieces(count, kSendMaxPerLaunch, [&](uint64_t f, uint64_t cnt) {
        return launch(send_jobs_kernel, grid256(cnt), dim3(256), s, rows, d_row_off, d_row_size, f, cnt, src_off, sizes,
                      first + 1);
      });
    if (rc != SF_OK) return rc;
    SF_HIP(hipMemcpyAsync(&missing, first + 1, 8, hipMemcpyDeviceToHost, s));
  }
  SF_HIP(hipStreamSynchronize(s));
  const int cls = sfwp::classify_get_block(tail, avail);
  // a whole message cannot stand where the device found none: the two test the same bytes
  if (cls == sfwp::kHeader) return SF_EIO;
  const uint64_t answered = std::min(missing, count);
  rc = build_run(d_src, src_len, reinterpret_cast<const uint8_t*>(table), src_off, sizes, answered, out, s);
  if (rc != SF_OK) return rc;
  *n_requests = count;
  *n_answered = answered;
  *consumed = at;
  *stop = cls;
  return SF_OK;
}

}  // namespace

extern "C" {

int sf_wire_block_data_device(const void* d_src, uint64_t src_len, const void* d_digests,
                              const uint64_t* d_src_offsets, const uint32_t* d_sizes, uint64_t n_blocks,
                              sf_wire_run** out, void* stream) {
  return guarded([&] {
    return build_run(static_cast<const uint8_t*>(d_src), src_len, static_cast<const uint8_t*>(d_digests),
                     d_src_offsets, d_sizes, n_blocks, out, as_stream(stream));
  });
}

int sf_serve_get_blocks_device(const sf_block_set* set, const uint64_t* d_row_offsets, const uint32_t* d_row_sizes,
                               const void* d_src, uint64_t src_len, const void* d_requests, uint64_t n_bytes,
                               sf_wire_run** out, uint64_t* n_requests, uint64_t* n_answered, uint64_t* consumed,
                               int* stop, void* stream) {
  return guarded([&] {
    return serve(set, d_row_offsets, d_row_sizes, static_cast<const uint8_t*>(d_src), src_len,
                 static_cast<const uint8_t*>(d_requests), n_bytes, out, n_requests, n_answered, consumed, stop,
                 as_stream(stream));
  });
}

int sf_wire_run_info(const sf_wire_run* run, const void** bytes, uint64_t* n_bytes, uint64_t* n_messages) {
  if (!run) return SF_EINVAL;
  if (bytes) *bytes = run->bytes;
  if (n_bytes) *n_bytes = run->n_bytes;
  if (n_messages) *n_messages = run->n_messages;
  return SF_OK;
}

int sf_wire_run_read(const sf_wire_run* run, uint64_t offset, void* out, uint64_t len) {
  if (!run) return SF_EINVAL;
  if (offset > run->n_bytes || len > run->n_bytes - offset) return SF_ERANGE;
  if (len == 0) return SF_OK;
  if (!out) return SF_EINVAL;
  int cur = 0;
  SF_HIP(hipGetDevice(&cur));
  if (cur != run->device) SF_HIP(hipSetDevice(run->device));
  hipError_t e = hipEventSynchronize(run->done);  // the run is complete behind it
  if (e == hipSuccess) e = hipMemcpy(out, run->bytes + offset, len, hipMemcpyDeviceToHost);
  if (cur != run->device) (void)hipSetDevice(cur);
  return hip_err(e);
}

int sf_wire_run_free(sf_wire_run* run, void* stream) {
  if (!run) return SF_OK;
  int rc = SF_OK;
  if (run->bytes) rc = hip_err(hipFreeAsync(run->bytes, as_stream(stream)));  // stream_free, with its error
  if (run->done) (void)hipEventDestroy(run->done);
  delete run;
  return rc;
}

}  // extern "C"
