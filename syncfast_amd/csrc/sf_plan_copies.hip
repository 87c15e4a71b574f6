// sf_plan_copies.hip -- the local half of the destination's GetFiles state on
// the device (include/syncfast_amd.h: sf_plan_copies_device).  For every
// FILE_BLOCK whose hash it already holds the reference's sink reads the block
// from its own file, writes it into the incoming temp file and records the row
// as present (src/sync/fs.rs:461-471).  Here the outputs of
// sf_receive_files_device stay in HBM and become, in one call, the copy list
// sf_copy_blocks_device takes and the row arrays sf_wire_get_blocks_device and
// sf_place_block_data_device take; every local block is hashed and compared
// with the digest the source announced before it is used.
// Its own translation unit: the other kernels' code objects stay as they are.
// The per-block rules are sf_plan_copies.hpp's, shared with the host test that
// executes them.  Random-access, latency-bound integer work: no MFMA, no LDS.
//
// Every dependency is a kernel boundary (no lane waits for another wave), and
// atomics go on counters only:
//
//   class    one lane per block: its class (sfpc::Class) and whether its
//            input is refused; the refusals, five classes and the candidates'
//            bytes are counted, one atomic per wave that has any.
//   scan     rocprim inclusive scan of "is a candidate", uint64; the
//            candidate count and the counters come back in one copy: read-back
//            one.  A refusal ends the call here (SF_ERANGE): nothing of the
//            caller's has been written.
//   -- with an arena to verify against, and a candidate --
//   compact  one lane per block: candidate i writes its place in the arena
//            and its size at entry scan - 1 of a list of the candidates alone.
//   hash     the explicit-list kernel over that list (sfi::launch_table).
//   verify   one lane per block: a candidate whose digest is the announced
//            one becomes a job, another is unverified; the unverified and the
//            jobs' bytes are counted.
//   scan     of "is a job"; the job count and the two counters: read-back two.
//   -- always --
//   emit     one lane per block: present, ask and dst of every block, entry
//            scan - 1 of the four job lists for a job, and one atomic per job
//            on its local file's counter.  A query, or a cap below the job
//            count, runs it for the counters alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/iterator/transform_iterator.hpp>

#include "sf_device.hpp"
#include "sf_launch.hpp"
#include "sf_plan_copies.hpp"
#include "../../include/syncfast_amd_test.h"

namespace {

constexpr uint64_t kMaxCount = 1ull << 31;  // one lane per block, one launch: the grid's x stays below 2^23

// What every kernel reads: the call's inputs.
struct PlanIn {
  const uint8_t* digests;
  const uint32_t* sizes;
  const uint64_t* offsets;
  const int64_t* rows;
  const uint32_t* block_file;
  uint64_t n;
  const uint64_t* file_base;
  uint64_t n_files;
  const uint32_t* table_file;
  const uint64_t* table_offset;
  const uint32_t* table_size;
  uint64_t n_table;
  const uint64_t* local_base;  // NULL: a query
  const uint64_t* local_size;
  uint64_t n_local;
  uint64_t src_len;
  int check_src;  // candidates must lie in [0, src_len)
};

// The counters behind the scan's end offsets, read back with its last entry.
enum Counter { C_BAD, C_MISSING, C_MISMATCH, C_STALE, C_UNAVAILABLE, C_EMPTY, C_CAND_BYTES, C_UNVERIFIED, C_JOB_BYTES,
               C_COUNT };

struct IsClass {
  uint8_t c;
  __host__ __device__ uint64_t operator()(uint8_t f) const { return f == c ? 1ull : 0ull; }
};

// The wave's lanes with `on`, added to *counter by one lane when there are
// any.  Every lane of the wave calls it.
__device__ __forceinline__ void count_wave(bool on, unsigned long long* counter) {
  const unsigned long long m = __ballot(on);
  if (m && (threadIdx.x & 63u) == 0) atomicAdd(counter, (unsigned long long)__popcll(m));
}

// The wave's sum of v, added to *counter by one lane when it is not 0.  Every
// lane of the wave calls it.
__device__ __forceinline__ void sum_wave(unsigned long long v, unsigned long long* counter) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  if (v && (threadIdx.x & 63u) == 0) atomicAdd(counter, v);
}

__global__ void __launch_bounds__(256) plan_class_kernel(PlanIn in, uint8_t* __restrict__ cls,
                                                         unsigned long long* __restrict__ ctr) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint8_t c = sfpc::kNone;
  bool bad = false;
  unsigned long long bytes = 0;
  if (i < in.n) {
    const int64_t r = in.rows[i];
    const uint32_t size = in.sizes[i], f = in.block_file[i];
    uint64_t dst = 0;
    bad = !sfpc::section_ok(f, in.n_files) || !sfpc::dst_of(in.file_base[f], in.offsets[i], &dst);
    c = sfpc::kMissing;
    if (!sfpc::row_ok(r, in.n_table)) {
      bad = true;
    } else if (r >= 0) {
      const uint32_t j = in.table_file[r];
      if (!sfpc::file_ok(j, in.n_local)) {
        bad = true;
      } else {
        const uint64_t at = in.table_offset[r], base = in.local_base ? in.local_base[j] : 0;
        c = sfpc::classify(r, size, in.table_size[r], at, in.local_size[j], base);
        if (c == sfpc::kCandidate) {
          if (in.check_src && !sfpc::in_arena(base, at, size, in.src_len)) bad = true;
          bytes = size;
        }
      }
    }
    cls[i] = c;
  }
  count_wave(bad, ctr + C_BAD);
  count_wave(c == sfpc::kMissing, ctr + C_MISSING);
  count_wave(c == sfpc::kSizeMismatch, ctr + C_MISMATCH);
  count_wave(c == sfpc::kStale, ctr + C_STALE);
  count_wave(c == sfpc::kUnavailable, ctr + C_UNAVAILABLE);
  count_wave(c == sfpc::kEmpty, ctr + C_EMPTY);
  sum_wave(bytes, ctr + C_CAND_BYTES);
}

// The candidates alone, in block order: where each lies in the arena, and its size.
__global__ void __launch_bounds__(256) plan_compact_kernel(PlanIn in, const uint8_t* __restrict__ cls,
                                                           const uint64_t* __restrict__ ends,
                                                           uint64_t* __restrict__ cand_off,
                                                           uint32_t* __restrict__ cand_size) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= in.n || cls[i] != sfpc::kCandidate) return;
  const uint64_t k = ends[i] - 1;
  const int64_t r = in.rows[i];
  cand_off[k] = in.local_base[in.table_file[r]] + in.table_offset[r];
  cand_size[k] = in.sizes[i];
}

// cand_digests[k]: what candidate k's bytes hash to.
__global__ void __launch_bounds__(256) plan_verify_kernel(const uint8_t* __restrict__ digests,
                                                          const uint32_t* __restrict__ sizes,
                                                          const uint8_t* __restrict__ cand_digests,
                                                          const uint64_t* __restrict__ ends, uint64_t n,
                                                          uint8_t* __restrict__ cls,
                                                          unsigned long long* __restrict__ ctr) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool unverified = false;
  unsigned long long bytes = 0;
  if (i < n && cls[i] == sfpc::kCandidate) {
    const uint32_t* want = reinterpret_cast<const uint32_t*>(digests + i * sfpc::kDigest);  // rows are 4-B aligned
    const uint32_t* got = reinterpret_cast<const uint32_t*>(cand_digests + (ends[i] - 1) * sfpc::kDigest);
    if (sfpc::same_digest(want, got)) {
      cls[i] = sfpc::kJob;
      bytes = sizes[i];
    } else {
      cls[i] = sfpc::kUnverified;
      unverified = true;
    }
  }
  count_wave(unverified, ctr + C_UNVERIFIED);
  sum_wave(bytes, ctr + C_JOB_BYTES);
}

// lists == 0: the local files' job counters alone.
__global__ void __launch_bounds__(256) plan_emit_kernel(PlanIn in, const uint8_t* __restrict__ cls,
                                                        const uint64_t* __restrict__ ends, uint8_t job_class,
                                                        int lists, uint8_t* __restrict__ present,
                                                        uint8_t* __restrict__ ask, uint64_t* __restrict__ dst,
                                                        uint64_t* __restrict__ src_off, uint64_t* __restrict__ dst_off,
                                                        uint32_t* __restrict__ job_sizes,
                                                        int64_t* __restrict__ job_blocks,
                                                        uint32_t* __restrict__ local_jobs) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= in.n) return;
  const uint8_t c = cls[i];
  uint64_t d = 0;
  if (lists) {
    (void)sfpc::dst_of(in.file_base[in.block_file[i]], in.offsets[i], &d);
    const bool here = sfpc::present(c, job_class);
    dst[i] = d;
    present[i] = here ? 1 : 0;
    ask[i] = here ? 0 : 1;
  }
  if (c != job_class) return;
  const int64_t r = in.rows[i];
  const uint32_t j = in.table_file[r];
  if (lists) {
    const uint64_t k = ends[i] - 1;
    src_off[k] = in.local_base[j] + in.table_offset[r];
    dst_off[k] = d;
    job_sizes[k] = in.sizes[i];
    job_blocks[k] = (int64_t)i;
  }
  if (local_jobs) atomicAdd(&local_jobs[j], 1u);
}

sfi::Stats4 g_plan_stats;  // sf_test_plan_copies_stats: read-backs, candidates hashed, jobs, 1 for a query

}  // namespace

using namespace sfi;

namespace {

using Flags = rocprim::transform_iterator<const uint8_t*, IsClass, uint64_t>;

// ends[i] = the entries of class c in cls[0 .. i]; tmp NULL: the temporary's size alone
int scan_class(void* tmp, size_t& tmp_bytes, const uint8_t* cls, uint8_t c, uint64_t* ends, uint64_t n,
               hipStream_t s) {
  return scan_inclusive(tmp, tmp_bytes, Flags(cls, IsClass{c}), ends, n, s);
}

struct Outs {
  uint8_t *present, *ask;
  uint64_t *dst, *src_off, *dst_off;
  uint32_t* job_sizes;
  int64_t* job_blocks;
  uint64_t cap;
  uint32_t* local_jobs;
};

int plan_copies(const PlanIn& in, const uint8_t* d_src, const Outs& o, uint64_t* counts, hipStream_t s) {
  g_plan_stats.reset();
  if (!counts) return SF_EINVAL;
  if (in.n > kMaxCount || in.n_files > kMaxCount || in.n_table > kMaxCount || in.n_local > kMaxCount)
    return SF_EINVAL;
  if (misaligned(in.digests, 4) || misaligned(in.sizes, 4) || misaligned(in.offsets, 8) || misaligned(in.rows, 8) ||
      misaligned(in.block_file, 4) || misaligned(in.file_base, 8) || misaligned(in.table_file, 4) ||
      misaligned(in.table_offset, 8) || misaligned(in.table_size, 4) || misaligned(in.local_base, 8) ||
      misaligned(in.local_size, 8) || misaligned(o.dst, 8) || misaligned(o.src_off, 8) || misaligned(o.dst_off, 8) ||
      misaligned(o.job_sizes, 4) || misaligned(o.job_blocks, 8) || misaligned(o.local_jobs, 4))
    return SF_EINVAL;
  const bool query = !in.local_base || !o.src_off || !o.dst_off || !o.job_sizes || !o.job_blocks;
  if (in.n) {
    if (!in.digests || !in.sizes || !in.offsets || !in.rows || !in.block_file) return SF_EINVAL;
    if ((in.n_files && !in.file_base) || (in.n_local && !in.local_size)) return SF_EINVAL;
    if (in.n_table && (!in.table_file || !in.table_offset || !in.table_size)) return SF_EINVAL;
    if (!query && (!o.present || !o.ask || !o.dst)) return SF_EINVAL;
  }
  if (in.n == 0) {
    if (o.local_jobs && in.n_local) SF_HIP(hipMemsetAsync(o.local_jobs, 0, in.n_local * 4, s));
    for (int k = 0; k < SF_PLAN_COUNTS; k++) counts[k] = 0;
    return SF_OK;
  }
  const uint64_t n = in.n;
  const bool verify = d_src && in.local_base;
  size_t tmp = 0;
  int rc = scan_class(nullptr, tmp, nullptr, 0, nullptr, n, s);
  if (rc != SF_OK) return rc;
  // end offsets with the counters behind them (read back together), the
  // blocks' classes, the scan's
  ScratchLayout L;
  const size_t ends_at = L.add((n + C_COUNT) * 8), cls_at = L.add(n);
  Scratch ws(s);
  rc = stream_alloc(&ws.p, L.total() + tmp + 8, s);
  if (rc != SF_OK) return rc;
  uint64_t* ends = L.at<uint64_t>(ws.p, ends_at);
  unsigned long long* ctr = reinterpret_cast<unsigned long long*>(ends + n);
  uint8_t* cls = L.at<uint8_t>(ws.p, cls_at);
  void* scan_tmp = L.at<void>(ws.p, L.total());
  SF_HIP(hipMemsetAsync(ctr, 0, C_COUNT * 8, s));
  PlanIn k_in = in;
  k_in.check_src = verify ? 1 : 0;
  rc = launch(plan_class_kernel, grid256(n), dim3(256), s, k_in, cls, ctr);
  if (rc == SF_OK) rc = scan_class(scan_tmp, tmp, cls, sfpc::kCandidate, ends, n, s);
  if (rc != SF_OK) return rc;
  uint64_t back[1 + C_COUNT] = {};  // the scan's last entry, then the counters
  SF_HIP(hipMemcpyAsync(back, ends + n - 1, (1 + C_CAND_BYTES + 1) * 8, hipMemcpyDeviceToHost, s));
  SF_HIP(hipStreamSynchronize(s));
  g_plan_stats.set(0, 1);
  if (back[1 + C_BAD]) return SF_ERANGE;
  const uint64_t candidates = back[0];
  uint64_t jobs = candidates, bytes = back[1 + C_CAND_BYTES], unverified = 0;
  uint8_t job_class = sfpc::kCandidate;

  Scratch vs(s);  // the candidates' list and digests: freed after the kernels that read them, in stream order
  if (verify && candidates) {
    ScratchLayout V;
    const size_t off_at = V.add(candidates * 8), dig_at = V.add(candidates * sfpc::kDigest),
                 size_at = V.add(candidates * 4);
    rc = stream_alloc(&vs.p, V.total(), s);
    if (rc != SF_OK) return rc;
    uint64_t* cand_off = V.at<uint64_t>(vs.p, off_at);
    uint8_t* cand_dig = V.at<uint8_t>(vs.p, dig_at);
    uint32_t* cand_size = V.at<uint32_t>(vs.p, size_at);
    rc = launch(plan_compact_kernel, grid256(n), dim3(256), s, k_in, cls, ends, cand_off, cand_size);
    if (rc == SF_OK) rc = launch_table(d_src, in.src_len, cand_off, cand_size, candidates, cand_dig, nullptr, s);
    if (rc == SF_OK)
      rc = launch(plan_verify_kernel, grid256(n), dim3(256), s, in.digests, in.sizes, cand_dig, ends, n, cls, ctr);
    if (rc == SF_OK) rc = scan_class(scan_tmp, tmp, cls, sfpc::kJob, ends, n, s);
    if (rc != SF_OK) return rc;
    SF_HIP(hipMemcpyAsync(back, ends + n - 1, (1 + C_COUNT) * 8, hipMemcpyDeviceToHost, s));
    SF_HIP(hipStreamSynchronize(s));
    g_plan_stats.set(0, 2);
    g_plan_stats.set(1, candidates);
    jobs = back[0], bytes = back[1 + C_JOB_BYTES], unverified = back[1 + C_UNVERIFIED];
    job_class = sfpc::kJob;
  }
  g_plan_stats.set(2, jobs);
  g_plan_stats.set(3, query ? 1 : 0);
  const bool lists = !query && jobs <= o.cap;
  if (o.local_jobs && in.n_local) SF_HIP(hipMemsetAsync(o.local_jobs, 0, in.n_local * 4, s));
  if (lists || (o.local_jobs && jobs)) {
    rc = launch(plan_emit_kernel, grid256(n), dim3(256), s, k_in, cls, ends, job_class, lists ? 1 : 0, o.present,
                o.ask, o.dst, o.src_off, o.dst_off, o.job_sizes, o.job_blocks, o.local_jobs);
    if (rc != SF_OK) return rc;
  }
  counts[SF_PLAN_JOBS] = jobs;
  counts[SF_PLAN_BYTES] = bytes;
  counts[SF_PLAN_MISSING] = back[1 + C_MISSING];
  counts[SF_PLAN_SIZE_MISMATCH] = back[1 + C_MISMATCH];
  counts[SF_PLAN_STALE] = back[1 + C_STALE];
  counts[SF_PLAN_UNAVAILABLE] = back[1 + C_UNAVAILABLE];
  counts[SF_PLAN_UNVERIFIED] = unverified;
  counts[SF_PLAN_EMPTY] = back[1 + C_EMPTY];
  return lists ? SF_OK : SF_ENOSPC;
}

}  // namespace

extern "C" {

int sf_plan_copies_device(const void* d_digests, const uint32_t* d_sizes, const uint64_t* d_offsets,
                          const int64_t* d_rows, const uint32_t* d_block_file, uint64_t n_blocks,
                          const uint64_t* d_file_base, uint64_t n_files, const uint32_t* d_table_file,
                          const uint64_t* d_table_offset, const uint32_t* d_table_size, uint64_t n_table,
                          const uint64_t* d_local_base, const uint64_t* d_local_size, uint64_t n_local,
                          const void* d_src, uint64_t src_len, uint8_t* d_present, uint8_t* d_ask, uint64_t* d_dst,
                          uint64_t* d_src_offsets, uint64_t* d_dst_offsets, uint32_t* d_job_sizes,
                          int64_t* d_job_blocks, uint64_t cap, uint32_t* d_local_jobs, uint64_t* counts,
                          void* stream) {
  return guarded([&] {
    const PlanIn in{static_cast<const uint8_t*>(d_digests), d_sizes, d_offsets, d_rows, d_block_file, n_blocks,
                    d_file_base, n_files, d_table_file, d_table_offset, d_table_size, n_table, d_local_base,
                    d_local_size, n_local, src_len, 0};
    const Outs o{d_present, d_ask, d_dst, d_src_offsets, d_dst_offsets, d_job_sizes, d_job_blocks, cap, d_local_jobs};
    return plan_copies(in, static_cast<const uint8_t*>(d_src), o, counts, as_stream(stream));
  });
}

int sf_test_plan_copies_stats(uint64_t out[4]) { return g_plan_stats.read(out); }

}  // extern "C"
