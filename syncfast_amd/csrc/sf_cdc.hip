// sf_cdc.hip -- the reference's content-defined (ZPAQ) block boundaries cut on
// the device (include/syncfast_amd.h: sf_cut_device_zpaq, sf_index_device_zpaq,
// sf_index_fd_zpaq).  Its own translation unit: the SHA-1 kernels' code objects
// stay as they are.
//
// The per-byte chain (sf_zpaq_step.hpp) is serial from each chunk's first
// byte, and the chunker restarts at every cut, so the boundaries are a
// function of where a chunk starts.  Parallelism comes from segments, as in
// sf_cut_fd's host join (sf_cut.cpp), with kernel boundaries as the only
// dependencies -- no kernel waits for another wave:
//
//   round 0   the buffer is split into segments of L bytes, L = the least
//             common multiple of max_size and 32 (a function of max_size
//             only; every full segment holds at least one cut, and a segment
//             owns whole words of the cut bitmaps).  One lane per segment
//             cuts it from its first byte with a fresh state and records, as
//             bits, the cuts that end in (s0, s0 + L] -- its speculative list.
//   join      segment s takes as its incoming cut the last cut of segment
//             s - 1's current list (of the previous round: the lists' last
//             cuts are double-buffered).  If that differs from the one it used
//             last, it cuts again from there with a fresh state until a cut
//             coincides with one of its round-0 cuts, adopts the rest of the
//             round-0 list from there, or keeps its own cuts if none
//             coincides before the segment ends.  The host reads one
//             changed-count per round and repeats until it is 0.  By
//             induction from segment 0 (whose round-0 list is true) the fixed
//             point is the sequential list, reached in at most nseg rounds.
//   compact   per-segment counts, a prefix sum, and one lane per segment
//             writes its (offset, size) rows in file order; the last block
//             ends at len.
//
// Every loop is bounded by a segment's length (+ max_size for a join's run-in),
// by len or by nseg.
//
// Constant or periodic data is serial in rounds: speculative and true cuts
// never coincide on it, so the join advances ONE segment per round
// (nseg - 1 rounds, one lane working in each).  The result stays exact; the
// time is that of a single lane walking the buffer plus a kernel boundary and
// a host read per segment (DESIGN.md 3.7 has the measured figure).
//
// Kernel shape: a wave per workgroup, a lane per segment.  Per lane h, c1, the
// run length and the 256-byte order-1 table in LDS (16 KiB per wave), laid out
// so that lane l only ever touches bank l mod 32: entry e of lane l is byte
// (e >> 2) * 256 + l * 4 + (e & 3).  Lanes read their own segments (stride L)
// 16 bytes at a time where the address allows, 64 bytes ahead of the bytes
// being fed.  The table's lookups and updates depend on the data only, not on
// h, so 16 bytes are fed with no branch (LaneChunker::feed16): the LDS
// traffic is one in-order stream beside the multiply chain, and a cut inside
// the 16 bytes is found afterwards (the table is wiped at a cut anyway).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <memory>

#include "host_sha1.h"
#include "sf_cdc_lane.hpp"
#include "sf_device.hpp"
#include "sf_launch.hpp"
#include "sf_stage.hpp"
#include "sf_zpaq_step.hpp"
#include "../../include/syncfast_amd_test.h"

namespace {

constexpr uint32_t kMinMaxSize = 16;      // device range of max_size
constexpr uint32_t kMaxMaxSize = 1u << 20;

struct Counters {
  unsigned long long recut;  // bytes cut again in joins (all rounds)
  uint32_t changed;          // segments that cut again this round
  uint32_t pad;
};

// LaneChunker (one lane's chunker, its order-1 table in LDS) and CutWriter (a
// segment's bitmap words): sf_cdc_lane.hpp, shared with sf_cdc_files.hip.

__global__ void __launch_bounds__(kLanes) zpaq_round0_kernel(const uint8_t* __restrict__ data, uint64_t len, uint64_t L,
                                                             uint64_t nseg, uint32_t lim, uint32_t max_size,
                                                             uint32_t* __restrict__ spec, uint32_t* __restrict__ cur,
                                                             uint64_t* __restrict__ last, uint64_t* __restrict__ lastspec,
                                                             uint64_t* __restrict__ used) {
  __shared__ uint8_t lds[kLanes * 256];
  const uint64_t s = (uint64_t)blockIdx.x * kLanes + threadIdx.x;
  if (s >= nseg) return;
  const uint64_t s0 = s * L, s1 = s0 + L < len ? s0 + L : len;
  LaneChunker z;
  z.tab = lds + threadIdx.x * 4;
  z.lim = lim;
  z.max_size = max_size;
  z.fresh();
  z.rpos = ~0ull;
  z.r0 = z.r1 = z.r2 = z.r3 = uint4{0, 0, 0, 0};
  CutWriter wr{spec, cur, s0 >> 5, 0u};
  uint64_t lastcut = s0;
  for (uint64_t p = s0; p < s1;) {
    bool cut;
    p = z.advance(data, p, s1, cut);
    if (cut) {
      wr.put(p - 1);
      lastcut = p;
    }
  }
  wr.finish((s1 - 1) >> 5);
  if (s1 == len) cur[(len - 1) >> 5] |= 1u << ((len - 1) & 31);  // the last block ends at len
  last[s] = lastcut;
  lastspec[s] = lastcut;
  used[s] = s0;
}

__global__ void __launch_bounds__(kLanes) zpaq_join_kernel(const uint8_t* __restrict__ data, uint64_t len, uint64_t L,
                                                           uint64_t nseg, uint32_t lim, uint32_t max_size,
                                                           const uint32_t* __restrict__ spec, uint32_t* __restrict__ cur,
                                                           const uint64_t* __restrict__ last_in,
                                                           uint64_t* __restrict__ last_out,
                                                           const uint64_t* __restrict__ lastspec,
                                                           uint64_t* __restrict__ used, Counters* __restrict__ ctr) {
  __shared__ uint8_t lds[kLanes * 256];
  const uint64_t s = (uint64_t)blockIdx.x * kLanes + threadIdx.x;
  if (s >= nseg) return;
  if (s == 0) {  // segment 0 starts at byte 0: its round-0 list is the true one
    last_out[0] = last_in[0];
    return;
  }
  const uint64_t inc = last_in[s - 1];  // in (s0 - max_size, s0]
  if (inc == used[s]) {
    last_out[s] = last_in[s];
    return;
  }
  used[s] = inc;
  atomicAdd(&ctr->changed, 1u);
  const uint64_t s0 = s * L, s1 = s0 + L < len ? s0 + L : len, wend = (s1 - 1) >> 5;
  LaneChunker z;
  z.tab = lds + threadIdx.x * 4;
  z.lim = lim;
  z.max_size = max_size;
  z.fresh();
  z.rpos = ~0ull;
  z.r0 = z.r1 = z.r2 = z.r3 = uint4{0, 0, 0, 0};
  CutWriter wr{cur, nullptr, s0 >> 5, 0u};
  uint64_t lastcut = inc, p = inc;
  bool synced = false;
  while (p < s1) {
    bool cut;
    p = z.advance(data, p, s1, cut);
    if (!cut || p <= s0) continue;  // no cut, or the run-in: the previous segment's bytes
    const uint64_t i = p - 1;
    wr.put(i);
    lastcut = p;
    if (spec[i >> 5] & (1u << (i & 31))) {  // one of the round-0 cuts: the rest of that list follows
      synced = true;
      break;
    }
  }
  if (synced) {
    const uint64_t i = p - 1, w = i >> 5;
    const uint32_t above = (i & 31) == 31 ? 0u : ~0u << ((i & 31) + 1);
    cur[w] = wr.acc | (spec[w] & above);
    for (uint64_t k = w + 1; k <= wend; k++) cur[k] = spec[k];
    lastcut = lastspec[s];
  } else {
    wr.finish(wend);
  }
  if (s1 == len) cur[(len - 1) >> 5] |= 1u << ((len - 1) & 31);  // the last block ends at len
  atomicAdd(&ctr->recut, (unsigned long long)(p - inc));
  last_out[s] = lastcut;
}

__global__ void __launch_bounds__(256) zpaq_count_kernel(const uint32_t* __restrict__ cur, uint64_t len, uint64_t L,
                                                         uint64_t nseg, uint64_t* __restrict__ counts) {
  const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nseg) return;
  const uint64_t s0 = s * L, s1 = s0 + L < len ? s0 + L : len;
  uint64_t n = 0;
  for (uint64_t w = s0 >> 5; w <= (s1 - 1) >> 5; w++) n += (uint64_t)__popc(cur[w]);
  counts[s] = n;
}

// ends[s] = number of blocks ending in segments 0..s (inclusive scan of the
// counts); segment s writes rows [ends[s - 1], ends[s]).  Its first block
// starts at the last cut of segment s - 1 (every full segment has one).
__global__ void __launch_bounds__(256) zpaq_emit_kernel(const uint32_t* __restrict__ cur, uint64_t len, uint64_t L,
                                                        uint64_t nseg, const uint64_t* __restrict__ ends,
                                                        const uint64_t* __restrict__ last, uint64_t* __restrict__ offsets,
                                                        uint32_t* __restrict__ sizes) {
  const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nseg) return;
  const uint64_t s0 = s * L, s1 = s0 + L < len ? s0 + L : len;
  uint64_t row = s ? ends[s - 1] : 0, prev = s ? last[s - 1] : 0;
  const uint64_t row_end = ends[s];
  for (uint64_t w = s0 >> 5; w <= (s1 - 1) >> 5; w++) {
    uint32_t m = cur[w];
    while (m && row < row_end) {
      const uint64_t end = (w << 5) + (uint64_t)__ffs((int)m);  // bit k set: ends after byte w * 32 + k
      m &= m - 1;
      offsets[row] = prev;
      sizes[row] = (uint32_t)(end - prev);
      prev = end;
      row++;
    }
  }
}

sfi::Stats4 g_last_stats;  // sf_test_zpaq_device_stats

inline uint64_t gcd64(uint64_t a, uint64_t b) {
  while (b) {
    const uint64_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}

}  // namespace

namespace sfi {

uint64_t zpaq_segment_len(uint32_t max_size) { return (uint64_t)max_size / gcd64(max_size, 32) * 32; }

int zpaq_check_device_params(uint32_t bits, uint32_t max_size) {
  return bits >= 1 && bits <= 31 && max_size >= kMinMaxSize && max_size <= kMaxMaxSize ? SF_OK : SF_EINVAL;
}

// The cut of d_data[0, len) (len > 0) up to the count: everything but the
// rows.  Blocking (one synchronisation of `s` per join round and one for the
// count).  The plan holds stream-ordered scratch until zpaq_cut_free.
int zpaq_cut_plan(const uint8_t* d_data, uint64_t len, uint32_t bits, uint32_t max_size, hipStream_t s, ZpaqPlan* p) {
  *p = ZpaqPlan{};
  const uint64_t L = zpaq_segment_len(max_size), nseg = ceil_div(len, L), nwords = ceil_div(len, 32);
  if (ceil_div(nseg, kLanes) > 0x7FFFFFFFull) return SF_EINVAL;
  size_t tmp = 0;
  uint64_t* const nul = nullptr;
  int rc = scan_inclusive(nullptr, tmp, nul, nul, nseg, s);
  if (rc != SF_OK) return rc;
  // two bitmaps of the cuts, six lists of one entry per segment, the counters, the scan's
  ScratchLayout lay;
  const size_t spec_at = lay.add(nwords * 4), cur_at = lay.add(nwords * 4);
  size_t seg_at[6];
  for (size_t& at : seg_at) at = lay.add(nseg * 8);
  const size_t ctr_at = lay.add(sizeof(Counters));
  if ((rc = stream_alloc(&p->ws, lay.total() + tmp + 8, s)) != SF_OK) return rc;
  uint32_t* spec = lay.at<uint32_t>(p->ws, spec_at);
  uint32_t* cur = lay.at<uint32_t>(p->ws, cur_at);
  uint64_t* seg[6];
  for (int k = 0; k < 6; k++) seg[k] = lay.at<uint64_t>(p->ws, seg_at[k]);
  uint64_t *last[2] = {seg[0], seg[1]}, *lastspec = seg[2], *used = seg[3], *counts = seg[4], *ends = seg[5];
  Counters* ctr = lay.at<Counters>(p->ws, ctr_at);
  const uint32_t lim = sfz::limit(bits);
  const dim3 grid((unsigned)ceil_div(nseg, kLanes)), block(kLanes);
  SF_HIP(hipMemsetAsync(ctr, 0, sizeof(Counters), s));
  rc = launch(zpaq_round0_kernel, grid, block, s, d_data, len, L, nseg, lim, max_size, spec, cur, last[0], lastspec,
              used);
  if (rc != SF_OK) return rc;
  uint64_t rounds = 0;
  int in = 0;
  Counters hc{};
  for (; nseg > 1; rounds++) {
    if (rounds > nseg) return SF_EIO;  // cannot happen: the fixed point is reached in nseg rounds
    SF_HIP(hipMemsetAsync(&ctr->changed, 0, sizeof(uint32_t), s));
    rc = launch(zpaq_join_kernel, grid, block, s, d_data, len, L, nseg, lim, max_size, spec, cur, last[in],
                last[in ^ 1], lastspec, used, ctr);
    if (rc != SF_OK) return rc;
    SF_HIP(hipMemcpyAsync(&hc, ctr, sizeof(Counters), hipMemcpyDeviceToHost, s));
    SF_HIP(hipStreamSynchronize(s));
    in ^= 1;
    if (hc.changed == 0) break;
  }
  rc = launch(zpaq_count_kernel, grid256(nseg), dim3(256), s, cur, len, L, nseg, counts);
  if (rc == SF_OK) rc = scan_inclusive(lay.at<void>(p->ws, lay.total()), tmp, counts, ends, nseg, s);
  if (rc != SF_OK) return rc;
  uint64_t total = 0;
  SF_HIP(hipMemcpyAsync(&total, ends + nseg - 1, 8, hipMemcpyDeviceToHost, s));
  SF_HIP(hipStreamSynchronize(s));
  p->len = len;
  p->L = L;
  p->nseg = nseg;
  p->total = total;
  p->cur = cur;
  p->ends = ends;
  p->last = last[in];
  g_last_stats.set(0, L);
  g_last_stats.set(1, nseg);
  g_last_stats.set(2, rounds);
  g_last_stats.set(3, hc.recut);
  return SF_OK;
}

// The rows of a plan: p.total entries at d_offsets / d_sizes.  Asynchronous.
int zpaq_cut_emit(const ZpaqPlan& p, uint64_t* d_offsets, uint32_t* d_sizes, hipStream_t s) {
  return launch(zpaq_emit_kernel, grid256(p.nseg), dim3(256), s, static_cast<const uint32_t*>(p.cur), p.len, p.L,
                p.nseg, static_cast<const uint64_t*>(p.ends), static_cast<const uint64_t*>(p.last), d_offsets, d_sizes);
}

void zpaq_cut_free(ZpaqPlan* p, hipStream_t s) {
  stream_free(p->ws, s);
  p->ws = nullptr;
}

}  // namespace sfi

using namespace sfi;

namespace {

// A plan's scratch goes back on every path out of a call.
struct PlanGuard {
  ZpaqPlan p;
  hipStream_t s;
  ~PlanGuard() { zpaq_cut_free(&p, s); }
};

int cut_device(const void* d_data, uint64_t len, uint32_t bits, uint32_t max_size, uint64_t* d_offsets,
               uint32_t* d_sizes, uint64_t cap_blocks, uint64_t* n_blocks, hipStream_t s) {
  if (n_blocks) *n_blocks = 0;
  if (!n_blocks || zpaq_check_device_params(bits, max_size) != SF_OK) return SF_EINVAL;
  if (misaligned(d_offsets, 8) || misaligned(d_sizes, 4)) return SF_EINVAL;  // zpaq_emit_kernel's stores
  if (len == 0) return SF_OK;
  if (!d_data) return SF_EINVAL;
  PlanGuard g{{}, s};
  int rc = zpaq_cut_plan(static_cast<const uint8_t*>(d_data), len, bits, max_size, s, &g.p);
  if (rc != SF_OK) return rc;
  *n_blocks = g.p.total;
  if (g.p.total > cap_blocks || !d_offsets || !d_sizes) return SF_ENOSPC;
  return zpaq_cut_emit(g.p, d_offsets, d_sizes, s);
}

constexpr uint64_t kFdPiece = 4ull << 20;  // bytes a reader thread reads, then copies to HBM, at a time

}  // namespace

// The windows of sf_index_fd_zpaq over the `len` bytes of the regular file open
// on fd: the rows into rb, folded into bh.
int sfi::fd_zpaq_windows(int fd, uint64_t len, uint32_t bits, uint32_t max_size, RowBuf& rb, sf_host_sha1_stream* bh) {
  int dev = 0;
  SF_HIP(hipGetDevice(&dev));
  // a window holds at least two chunks, so dropping its last one leaves one
  const int64_t wk = knob(K_TEST_ZPAQ_WINDOW);
  const uint64_t W = std::max<uint64_t>(wk > 0 ? (uint64_t)wk : kCacheMax, 2ull * max_size);
  HostLease res;
  hipStream_t* st;
  hipEvent_t* ev;
  uint8_t *pin = nullptr, *dwin = nullptr;
  const uint64_t wbytes = std::min(len, W);
  int rc = res.streams(st, ev);
  if (rc == SF_OK) rc = res.pin(kSlotData, wbytes, reinterpret_cast<void**>(&pin));
  if (rc == SF_OK) rc = res.dev(kSlotData, wbytes, reinterpret_cast<void**>(&dwin));
  if (rc != SF_OK) return rc;
  hipStream_t s = st[0];
  uint64_t w = 0;
  for (uint64_t A = 0; A < len; w++) {
    const uint64_t B = std::min(len, A + W), n_bytes = B - A;
    const bool eof = B == len;
    // the window, read once: each reader thread takes pieces, and a piece's
    // copy to HBM starts as soon as it is in the pinned window
    const uint64_t pieces = ceil_div(n_bytes, kFdPiece);
    std::atomic<uint64_t> next{0};
    std::atomic<int> fail{SF_OK};
    run_pool((unsigned)std::min<uint64_t>(io_threads(), pieces), [&] {
      if (hipSetDevice(dev) != hipSuccess) {
        (void)hipGetLastError();
        fail.store(SF_ENODEV);
        return;
      }
      for (uint64_t k; (k = next.fetch_add(1)) < pieces;) {
        const uint64_t o = k * kFdPiece, m = std::min(kFdPiece, n_bytes - o);
        if (!read_fully(fd, pin + o, A + o, m)) {  // an error, or the file shrank
          fail.store(SF_EIO);
          return;
        }
        if (hipMemcpyAsync(dwin + o, pin + o, m, hipMemcpyHostToDevice, s) != hipSuccess) {
          (void)hipGetLastError();
          fail.store(SF_ENODEV);
          return;
        }
      }
    });
    rc = fail.load();
    read_hook(w);
    if (rc != SF_OK) return rc;
    PlanGuard g{{}, s};
    if ((rc = zpaq_cut_plan(dwin, n_bytes, bits, max_size, s, &g.p)) != SF_OK) return rc;
    // a non-final window's last block was closed by the window's end, not by
    // the chunker: it is dropped, and the next window starts at its offset
    // (a true cut)
    const uint64_t n = g.p.total, keep = eof ? n : n - 1;
    const uint64_t lbytes = n * kListEntry;
    StageBufs sb;
    if ((rc = stage_bufs(res, 0, kNoBuf, n, lbytes, &sb)) != SF_OK) return rc;
    uint64_t* d_off = static_cast<uint64_t*>(sb.daux);
    uint32_t* d_sz = reinterpret_cast<uint32_t*>(d_off + n);
    if ((rc = zpaq_cut_emit(g.p, d_off, d_sz, s)) != SF_OK) return rc;
    if (keep && (rc = launch_table(dwin, n_bytes, d_off, d_sz, keep, sb.ddig, nullptr, s)) != SF_OK) return rc;
    SF_HIP(hipMemcpyAsync(sb.paux, sb.daux, lbytes, hipMemcpyDeviceToHost, s));
    if (keep) SF_HIP(hipMemcpyAsync(sb.pdig, sb.ddig, keep * 20, hipMemcpyDeviceToHost, s));
    SF_HIP(hipStreamSynchronize(s));
    if (!append_window_rows(rb, A, sb.paux, sb.pdig, n, keep, bh)) return SF_ENOMEM;
    if (eof) break;
    if (keep == 0) return SF_EIO;  // cannot happen: W >= 2 * max_size
    A += static_cast<const uint64_t*>(sb.paux)[n - 1];
  }
  return SF_OK;
}

namespace {

int index_fd_zpaq_body(int fd, const sf_file_stamp* expect, uint32_t bits, uint32_t max_size, sf_block_sig** rows,
                       uint64_t* n_out, uint8_t* blocks_hash) {
  if (rows) *rows = nullptr;
  if (n_out) *n_out = 0;
  if (fd < 0 || !rows || !n_out || !blocks_hash || zpaq_check_device_params(bits, max_size) != SF_OK)
    return SF_EINVAL;
  RowBuf rb;
  sf_host_sha1_stream bh;
  sf_host_sha1_begin(&bh);
  // (rows that end while the file is written are not one version's rows: SF_EAGAIN)
  const int rc = stamped(fd, expect, [&](const sf_file_stamp& before, mode_t mode) {
    if (!S_ISREG(mode)) return SF_EINVAL;
    return before.size ? fd_zpaq_windows(fd, before.size, bits, max_size, rb, &bh) : SF_OK;
  });
  if (rc != SF_OK) return rc;
  if (!rb.grow(1)) return SF_ENOMEM;  // no rows: still a pointer that free() takes
  sf_host_sha1_final(&bh, blocks_hash);
  *n_out = rb.n;
  *rows = rb.release();
  return SF_OK;
}

}  // namespace

extern "C" {

int sf_cut_device_zpaq(const void* d_data, uint64_t len, uint32_t bits, uint32_t max_size, uint64_t* d_offsets,
                       uint32_t* d_sizes, uint64_t cap_blocks, uint64_t* n_blocks, void* stream) {
  return guarded(
      [&] { return cut_device(d_data, len, bits, max_size, d_offsets, d_sizes, cap_blocks, n_blocks, as_stream(stream)); });
}

int sf_index_device_zpaq(const void* d_data, uint64_t len, uint32_t bits, uint32_t max_size, uint64_t* d_offsets,
                         uint32_t* d_sizes, void* d_digests, uint64_t cap_blocks, uint64_t* n_blocks,
                         uint8_t* blocks_hash, void* stream) {
  return guarded([&]() -> int {
    hipStream_t s = as_stream(stream);
    if (misaligned(d_digests, 4)) {  // digests are written as dwords (Sha1::store)
      if (n_blocks) *n_blocks = 0;
      return SF_EINVAL;
    }
    int rc = cut_device(d_data, len, bits, max_size, d_offsets, d_sizes, cap_blocks, n_blocks, s);
    if (rc != SF_OK) return rc;
    const uint64_t n = *n_blocks;
    if (n && !d_digests) return SF_EINVAL;
    if (n && (rc = launch_table(d_data, len, d_offsets, d_sizes, n, d_digests, nullptr, s)) != SF_OK) return rc;
    if (!blocks_hash) return SF_OK;
    std::vector<uint8_t> dig(n * 20);
    if (n) {
      SF_HIP(hipMemcpyAsync(dig.data(), d_digests, n * 20, hipMemcpyDeviceToHost, s));
      SF_HIP(hipStreamSynchronize(s));
    }
    return sf_blocks_hash(dig.data(), n, blocks_hash);
  });
}

int sf_index_fd_zpaq(int fd, const sf_file_stamp* expect, uint32_t bits, uint32_t max_size, sf_block_sig** rows,
                     uint64_t* n_out, uint8_t blocks_hash[SF_HASH_DIGEST_LEN]) {
  return guarded([&] { return index_fd_zpaq_body(fd, expect, bits, max_size, rows, n_out, blocks_hash); });
}

int sf_test_zpaq_device_stats(uint64_t out[4]) { return g_last_stats.read(out); }

}  // extern "C"
