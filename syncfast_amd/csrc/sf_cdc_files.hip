// sf_cdc_files.hip -- the device ZPAQ cut over MANY files in one call
// (include/syncfast_amd.h: sf_cut_device_zpaq_files,
// sf_index_device_zpaq_files).  Its own translation unit: sf_cdc.hip's
// kernels, and every other code object, stay as they are.
//
// These are sf_cdc.hip's four kernels (round 0, join, count, emit; its file
// comment explains the method and the LDS layout) with per-file geometry;
// nothing is new per byte.  The lane code -- LaneChunker, CutWriter -- is
// sf_cdc_lane.hpp, shared with sf_cdc.hip; all geometry is
// sf_cdc_files_plan.hpp, host arithmetic that tests/native/cdc_files_plan.cpp
// executes on a CPU.
//
// One buffer that is one file is latency-bound until it has about 131,072
// segments.  A batch of files supplies them: every file starts with a fresh
// chunker, so segments of different files never join, and a lane's work is
// the same whether its neighbours cut the same file or 63 others.  Each lane
// works on its file as if it were the whole buffer: its data pointer is the
// file's first byte, its bitmaps start at the file's word-aligned base, and
// every position it keeps (last, lastspec, used) is relative to the file.
//
// Finding a lane's file: a search of seg_first[] once per lane
// (sfzf::file_of, at most 32 dependent loads of an array that stays in L2)
// rather than a per-segment file index.  The index would cost 4 more bytes of
// scratch per segment and a kernel to fill it, to save a few hundred cycles
// in lanes that then feed at least one segment (up to L + max_size bytes, a
// dependent multiply per byte) each; for a tree of tiny files, where a lane's
// segment is short, the search is also short (it is over files, not bytes).
//
// The round cap.  Constant or periodic data joins one segment per round, so
// one sparse file in a batch would hold every other file for thousands of
// rounds.  The join kernel of launch r stores r at round[f] for every segment
// of file f that cuts again -- a plain vector store; all writers of a launch
// store the same value.  The host makes at most max_rounds launches (0: no
// cap), stopping early when a launch changes nothing.  A file whose round[f]
// equals the number of launches made cut again in the last one and is
// UNSETTLED: its counts are forced to 0, it emits no rows, and the caller
// finishes it another way.  Every other file is final (a segment can only
// change in launch r + 1 if its predecessor changed in launch r).
//
// Every loop is bounded by a segment's length (+ max_size for a join's
// run-in), by a file's length, by the segment count or by max_rounds; no
// kernel waits for another wave.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "sf_cdc_files_plan.hpp"
#include "sf_cdc_lane.hpp"
#include "sf_device.hpp"
#include "sf_launch.hpp"
#include "sf_zpaq_step.hpp"
#include "../../include/syncfast_amd_test.h"

namespace {

struct Counters {
  unsigned long long recut;  // bytes cut again in joins (all launches)
  uint32_t changed;          // segments that cut again in this launch
  uint32_t pad;
};

// The batch as the kernels see it (device arrays; sf_cdc_files_plan.hpp).
struct Files {
  const uint64_t* off;         // [n] first byte of file f in the buffer
  const uint64_t* len;         // [n]
  const uint64_t* seg_first;   // [n + 1]
  const uint64_t* word_first;  // [n + 1]
  uint32_t n;
};

__global__ void __launch_bounds__(kLanes) zpaq_files_round0_kernel(const uint8_t* __restrict__ data, Files F, uint64_t L,
                                                                   uint64_t nseg, uint32_t lim, uint32_t max_size,
                                                                   uint32_t* __restrict__ spec, uint32_t* __restrict__ cur,
                                                                   uint64_t* __restrict__ last,
                                                                   uint64_t* __restrict__ lastspec,
                                                                   uint64_t* __restrict__ used) {
  __shared__ uint8_t lds[kLanes * 256];
  const uint64_t s = (uint64_t)blockIdx.x * kLanes + threadIdx.x;
  if (s >= nseg) return;
  const uint32_t f = sfzf::file_of(F.seg_first, F.n, s);
  const uint64_t len = F.len[f], wbase = F.word_first[f];
  const sfzf::Seg g = sfzf::segment(f, F.seg_first[f], len, L, s);
  const uint8_t* __restrict__ fdata = data + F.off[f];
  const uint64_t s0 = g.s0, s1 = g.s1;
  LaneChunker z;
  z.tab = lds + threadIdx.x * 4;
  z.lim = lim;
  z.max_size = max_size;
  z.fresh();
  z.rpos = ~0ull;
  z.r0 = z.r1 = z.r2 = z.r3 = uint4{0, 0, 0, 0};
  CutWriter wr{spec + wbase, cur + wbase, g.w0, 0u};
  uint64_t lastcut = s0;
  for (uint64_t p = s0; p < s1;) {
    bool cut;
    p = z.advance(fdata, p, s1, cut);
    if (cut) {
      wr.put(p - 1);
      lastcut = p;
    }
  }
  wr.finish(g.wend);
  if (g.last(len)) cur[wbase + ((len - 1) >> 5)] |= 1u << ((len - 1) & 31);  // the file's last block ends at len
  last[s] = lastcut;
  lastspec[s] = lastcut;
  used[s] = s0;
}

__global__ void __launch_bounds__(kLanes) zpaq_files_join_kernel(const uint8_t* __restrict__ data, Files F, uint64_t L,
                                                                 uint64_t nseg, uint32_t lim, uint32_t max_size,
                                                                 const uint32_t* __restrict__ spec,
                                                                 uint32_t* __restrict__ cur,
                                                                 const uint64_t* __restrict__ last_in,
                                                                 uint64_t* __restrict__ last_out,
                                                                 const uint64_t* __restrict__ lastspec,
                                                                 uint64_t* __restrict__ used, uint32_t* __restrict__ round,
                                                                 uint32_t r, Counters* __restrict__ ctr) {
  __shared__ uint8_t lds[kLanes * 256];
  const uint64_t s = (uint64_t)blockIdx.x * kLanes + threadIdx.x;
  if (s >= nseg) return;
  const uint32_t f = sfzf::file_of(F.seg_first, F.n, s);
  const uint64_t len = F.len[f];
  const sfzf::Seg g = sfzf::segment(f, F.seg_first[f], len, L, s);
  if (g.first()) {  // a file's segment 0 starts at its byte 0: its round-0 list is the true one
    last_out[s] = last_in[s];
    return;
  }
  const uint64_t inc = last_in[sfzf::incoming_from(s)];  // in (s0 - max_size, s0], of the same file
  if (inc == used[s]) {
    last_out[s] = last_in[s];
    return;
  }
  used[s] = inc;
  round[f] = r;  // every writer of this launch stores r
  atomicAdd(&ctr->changed, 1u);
  const uint8_t* __restrict__ fdata = data + F.off[f];
  const uint32_t* __restrict__ fspec = spec + F.word_first[f];
  uint32_t* __restrict__ fcur = cur + F.word_first[f];
  const uint64_t s0 = g.s0, s1 = g.s1, wend = g.wend;
  LaneChunker z;
  z.tab = lds + threadIdx.x * 4;
  z.lim = lim;
  z.max_size = max_size;
  z.fresh();
  z.rpos = ~0ull;
  z.r0 = z.r1 = z.r2 = z.r3 = uint4{0, 0, 0, 0};
  CutWriter wr{fcur, nullptr, g.w0, 0u};
  uint64_t lastcut = inc, p = inc;
  bool synced = false;
  while (p < s1) {
    bool cut;
    p = z.advance(fdata, p, s1, cut);
    if (!cut || p <= s0) continue;  // no cut, or the run-in: the previous segment's bytes
    const uint64_t i = p - 1;
    wr.put(i);
    lastcut = p;
    if (fspec[i >> 5] & (1u << (i & 31))) {  // one of the round-0 cuts: the rest of that list follows
      synced = true;
      break;
    }
  }
  if (synced) {
    const uint64_t i = p - 1, w = i >> 5;
    fcur[w] = wr.acc | (fspec[w] & sfzf::above_bit(i));
    for (uint64_t k = w + 1; k <= wend; k++) fcur[k] = fspec[k];
    lastcut = lastspec[s];
  } else {
    wr.finish(wend);
  }
  if (g.last(len)) fcur[(len - 1) >> 5] |= 1u << ((len - 1) & 31);  // the file's last block ends at len
  atomicAdd(&ctr->recut, (unsigned long long)(p - inc));
  last_out[s] = lastcut;
}

// counts[s] = cuts in the words segment s owns; 0 for an unsettled file.
__global__ void __launch_bounds__(256) zpaq_files_count_kernel(const uint32_t* __restrict__ cur, Files F, uint64_t L,
                                                               uint64_t nseg, const uint32_t* __restrict__ round,
                                                               uint32_t launches, uint64_t* __restrict__ counts) {
  const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nseg) return;
  const uint32_t f = sfzf::file_of(F.seg_first, F.n, s);
  uint64_t n = 0;
  if (!sfzf::unsettled(round[f], launches)) {
    const sfzf::Seg g = sfzf::segment(f, F.seg_first[f], F.len[f], L, s);
    const uint32_t* __restrict__ fcur = cur + F.word_first[f];
    for (uint64_t w = g.w0; w <= g.wend; w++) n += (uint64_t)__popc(fcur[w]);
  }
  counts[s] = n;
}

// ends[] = the inclusive scan of counts[]; segment s writes rows
// [row_base(s), ends[s]).  Its first block starts at the last cut of the
// file's segment before it (every full segment has one), or at the file's
// byte 0.  Offsets are positions in the buffer.
__global__ void __launch_bounds__(256) zpaq_files_emit_kernel(const uint32_t* __restrict__ cur, Files F, uint64_t L,
                                                              uint64_t nseg, const uint64_t* __restrict__ ends,
                                                              const uint64_t* __restrict__ last,
                                                              uint64_t* __restrict__ offsets, uint32_t* __restrict__ sizes) {
  const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nseg) return;
  uint64_t row = sfzf::row_base(ends, s);
  const uint64_t row_end = ends[s];
  if (row == row_end) return;  // no cut ends here, or an unsettled file
  const uint32_t f = sfzf::file_of(F.seg_first, F.n, s);
  const sfzf::Seg g = sfzf::segment(f, F.seg_first[f], F.len[f], L, s);
  const uint32_t* __restrict__ fcur = cur + F.word_first[f];
  const uint64_t base = F.off[f];
  uint64_t prev = g.first() ? 0 : last[sfzf::incoming_from(s)];
  for (uint64_t w = g.w0; w <= g.wend; w++) {
    uint32_t m = fcur[w];
    while (m && row < row_end) {
      const uint64_t end = (w << 5) + (uint64_t)__ffs((int)m);  // bit k set: ends after byte w * 32 + k
      m &= m - 1;
      offsets[row] = base + prev;
      sizes[row] = (uint32_t)(end - prev);
      prev = end;
      row++;
    }
  }
}

// first_row[f], f = 0 .. n (the total).
__global__ void __launch_bounds__(256) zpaq_files_first_row_kernel(const uint64_t* __restrict__ seg_first,
                                                                   const uint64_t* __restrict__ ends, uint32_t n,
                                                                   uint64_t* __restrict__ first_row) {
  const uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f > n) return;
  first_row[f] = sfzf::first_row(seg_first, ends, (uint32_t)f);
}

// sf_test_zpaq_files_stats: L, segments, join launches, bytes cut again,
// unsettled files, files finished on the host.
std::atomic<uint64_t> g_files_stats[6];

}  // namespace

namespace sfi {

void zpaq_files_stat(int k, uint64_t v) { g_files_stats[k].store(v, std::memory_order_relaxed); }

int zpaq_files_check(uint64_t data_len, const uint64_t* offs, const uint64_t* lens, uint32_t n, uint32_t* bad_file) {
  for (uint32_t f = 0; f < n; f++)
    if (!sfzf::in_range(offs[f], lens[f], data_len)) {
      if (bad_file) *bad_file = f;
      return SF_ERANGE;
    }
  return SF_OK;
}

// The cut of the n files (checked: zpaq_files_check; at least one not empty)
// up to the count -- everything but the rows -- in two parts.
// zpaq_files_begin: the plan's scratch, the upload of the per-file arrays and
// round 0, the largest share of the cut.  Asynchronous on `s`; p->host must
// live until the stream has run past the upload.
int zpaq_files_begin(const uint8_t* d_data, const uint64_t* offs, const uint64_t* lens, uint32_t n, uint32_t bits,
                     uint32_t max_size, hipStream_t s, ZpaqFilesPlan* p) {
  const uint64_t L = zpaq_segment_len(max_size);
  // the four per-file arrays, uploaded in one copy: off, len, seg_first, word_first
  std::vector<uint64_t>& h = p->host;
  h.resize(4 * (size_t)n + 2);
  uint64_t *h_off = h.data(), *h_len = h_off + n, *h_seg = h_len + n, *h_word = h_seg + n + 1;
  memcpy(h_off, offs, (size_t)n * 8);
  memcpy(h_len, lens, (size_t)n * 8);
  sfzf::fill_firsts(lens, n, L, h_seg, h_word);
  const uint64_t nseg = h_seg[n], nwords = h_word[n];
  uint64_t most = 0;  // segments of the file that has most
  for (uint32_t f = 0; f < n; f++) most = std::max(most, h_seg[f + 1] - h_seg[f]);
  if (nseg == 0 || ceil_div(nseg, kLanes) > 0x7FFFFFFFull) return SF_EINVAL;
  size_t tmp = 0;
  uint64_t* const nul = nullptr;
  int rc = scan_inclusive(nullptr, tmp, nul, nul, nseg, s);
  if (rc != SF_OK) return rc;
  // two bitmaps of the cuts, six lists of one entry per segment, the counters,
  // the per-file arrays and round numbers, the scan's
  ScratchLayout lay;
  const size_t spec_at = lay.add(nwords * 4), cur_at = lay.add(nwords * 4);
  size_t seg_at[6];
  for (size_t& at : seg_at) at = lay.add(nseg * 8);
  const size_t ctr_at = lay.add(sizeof(Counters)), files_at = lay.add(h.size() * 8), round_at = lay.add((size_t)n * 4);
  if ((rc = stream_alloc(&p->ws, lay.total() + tmp + 8, s)) != SF_OK) return rc;
  p->spec = lay.at<void>(p->ws, spec_at);
  p->cur = lay.at<void>(p->ws, cur_at);
  for (int k = 0; k < 6; k++) p->seg[k] = lay.at<void>(p->ws, seg_at[k]);
  p->ctr = lay.at<void>(p->ws, ctr_at);
  p->d_files = lay.at<void>(p->ws, files_at);
  p->round = lay.at<void>(p->ws, round_at);
  p->scan_tmp = lay.at<void>(p->ws, lay.total());
  p->scan_bytes = tmp;
  p->d_data = d_data;
  p->L = L;
  p->nseg = nseg;
  p->most = most;
  p->n_files = n;
  p->bits = bits;
  p->max_size = max_size;
  uint64_t* d_files = static_cast<uint64_t*>(p->d_files);
  const Files F{d_files, d_files + n, d_files + 2 * (size_t)n, d_files + 3 * (size_t)n + 1, n};
  SF_HIP(hipMemcpyAsync(d_files, h.data(), h.size() * 8, hipMemcpyHostToDevice, s));
  SF_HIP(hipMemsetAsync(p->ctr, 0, sizeof(Counters), s));
  SF_HIP(hipMemsetAsync(p->round, 0, (size_t)n * 4, s));
  return launch(zpaq_files_round0_kernel, dim3((unsigned)ceil_div(nseg, kLanes)), dim3(kLanes), s, d_data, F, L, nseg,
                sfz::limit(bits), max_size, static_cast<uint32_t*>(p->spec), static_cast<uint32_t*>(p->cur),
                static_cast<uint64_t*>(p->seg[0]), static_cast<uint64_t*>(p->seg[2]), static_cast<uint64_t*>(p->seg[3]));
}

// zpaq_files_finish: the join launches (at most max_rounds; 0 = no cap), the
// count and the unsettled files of a plan begun on `s`.  Blocking: one
// synchronisation of `s` per join launch and one for the count.
int zpaq_files_finish(ZpaqFilesPlan* p, uint32_t max_rounds, hipStream_t s) {
  const uint32_t n = p->n_files;
  const uint64_t nseg = p->nseg, L = p->L;
  uint64_t* d_files = static_cast<uint64_t*>(p->d_files);
  const Files F{d_files, d_files + n, d_files + 2 * (size_t)n, d_files + 3 * (size_t)n + 1, n};
  const uint8_t* d_data = static_cast<const uint8_t*>(p->d_data);
  uint32_t *spec = static_cast<uint32_t*>(p->spec), *cur = static_cast<uint32_t*>(p->cur);
  uint64_t* seg[6];
  for (int k = 0; k < 6; k++) seg[k] = static_cast<uint64_t*>(p->seg[k]);
  uint64_t *last[2] = {seg[0], seg[1]}, *lastspec = seg[2], *used = seg[3], *counts = seg[4], *ends = seg[5];
  Counters* ctr = static_cast<Counters*>(p->ctr);
  uint32_t* round = static_cast<uint32_t*>(p->round);
  const uint32_t lim = sfz::limit(p->bits);
  const dim3 grid((unsigned)ceil_div(nseg, kLanes)), block(kLanes);
  uint32_t launches = 0;
  int in = 0, rc;
  Counters hc{};
  while (p->most > 1 && (max_rounds == 0 || launches < max_rounds)) {
    if (launches > p->most) return SF_EIO;  // cannot happen: a file's fixed point is reached in as many rounds as it has segments
    SF_HIP(hipMemsetAsync(&ctr->changed, 0, sizeof(uint32_t), s));
    rc = launch(zpaq_files_join_kernel, grid, block, s, d_data, F, L, nseg, lim, p->max_size, spec, cur, last[in],
                last[in ^ 1], lastspec, used, round, launches + 1, ctr);
    if (rc != SF_OK) return rc;
    SF_HIP(hipMemcpyAsync(&hc, ctr, sizeof(Counters), hipMemcpyDeviceToHost, s));
    SF_HIP(hipStreamSynchronize(s));
    p->synced = true;
    launches++;
    in ^= 1;
    if (hc.changed == 0) break;
  }
  rc = launch(zpaq_files_count_kernel, grid256(nseg), dim3(256), s, cur, F, L, nseg, round, launches, counts);
  if (rc == SF_OK) rc = scan_inclusive(p->scan_tmp, p->scan_bytes, counts, ends, nseg, s);
  if (rc != SF_OK) return rc;
  uint64_t total = 0;
  SF_HIP(hipMemcpyAsync(&total, ends + nseg - 1, 8, hipMemcpyDeviceToHost, s));
  p->unsettled.assign(n, 0);
  p->n_unsettled = 0;
  std::vector<uint32_t> h_round;
  if (hc.changed != 0) {  // the cap ended the loop: the files that cut again in the last launch
    h_round.resize(n);
    SF_HIP(hipMemcpyAsync(h_round.data(), round, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  }
  SF_HIP(hipStreamSynchronize(s));
  p->synced = true;
  for (uint32_t f = 0; f < n && !h_round.empty(); f++)
    if (sfzf::unsettled(h_round[f], launches)) {
      p->unsettled[f] = 1;
      p->n_unsettled++;
    }
  p->total = total;
  p->launches = launches;
  p->recut = hc.recut;
  p->ends = ends;
  p->last = last[in];
  return SF_OK;
}

// The rows of a plan: p.total entries at d_offsets / d_sizes, n_files + 1 at
// d_first_row.  Asynchronous.
int zpaq_files_emit(const ZpaqFilesPlan& p, uint64_t* d_offsets, uint32_t* d_sizes, uint64_t* d_first_row,
                    hipStream_t s) {
  const uint32_t n = p.n_files;
  const uint64_t* d_files = static_cast<const uint64_t*>(p.d_files);
  const Files F{d_files, d_files + n, d_files + 2 * (size_t)n, d_files + 3 * (size_t)n + 1, n};
  int rc = launch(zpaq_files_first_row_kernel, grid256((uint64_t)n + 1), dim3(256), s, F.seg_first,
                  static_cast<const uint64_t*>(p.ends), n, d_first_row);
  if (rc != SF_OK || p.total == 0) return rc;
  return launch(zpaq_files_emit_kernel, grid256(p.nseg), dim3(256), s, static_cast<const uint32_t*>(p.cur), F, p.L,
                p.nseg, static_cast<const uint64_t*>(p.ends), static_cast<const uint64_t*>(p.last), d_offsets, d_sizes);
}

void zpaq_files_free(ZpaqFilesPlan* p, hipStream_t s) {
  stream_free(p->ws, s);
  p->ws = nullptr;
}

}  // namespace sfi

using namespace sfi;

namespace {

// A plan's scratch goes back on every path out of a call -- on an early error
// only after the stream has run past the upload of the plan's host arrays.
struct FilesPlanGuard {
  ZpaqFilesPlan p;
  hipStream_t s;
  ~FilesPlanGuard() {
    if (p.ws && !p.synced) (void)hipStreamSynchronize(s);
    zpaq_files_free(&p, s);
  }
};

// have_rest: the caller's further device outputs are there (sf_index_device_zpaq_files' d_digests)
int cut_files(const void* d_data, uint64_t data_len, const uint64_t* offs, const uint64_t* lens, uint32_t n,
              uint32_t bits, uint32_t max_size, uint32_t max_rounds, uint64_t* d_offsets, uint32_t* d_sizes,
              uint64_t cap_blocks, uint64_t* d_first_row, bool have_rest, uint64_t* n_blocks, uint8_t* unsettled,
              uint32_t* n_unsettled, uint32_t* bad_file, hipStream_t s) {
  if (n_blocks) *n_blocks = 0;
  if (n_unsettled) *n_unsettled = 0;
  if (bad_file) *bad_file = 0;
  if (!n_blocks || zpaq_check_device_params(bits, max_size) != SF_OK || (n && (!offs || !lens))) return SF_EINVAL;
  if (misaligned(d_offsets, 8) || misaligned(d_first_row, 8) || misaligned(d_sizes, 4)) return SF_EINVAL;  // the emit kernels' stores
  int rc = zpaq_files_check(data_len, offs, lens, n, bad_file);
  if (rc != SF_OK) return rc;
  if (unsettled && n) memset(unsettled, 0, n);
  bool any = false;
  for (uint32_t f = 0; f < n && !any; f++) any = lens[f] != 0;
  if (!any) {  // no block: no device is needed unless first_row is asked for
    for (int k = 0; k < 6; k++) zpaq_files_stat(k, 0);
    if (d_first_row) SF_HIP(hipMemsetAsync(d_first_row, 0, ((size_t)n + 1) * 8, s));
    return SF_OK;
  }
  if (!d_data) return SF_EINVAL;
  FilesPlanGuard g{{}, s};
  rc = zpaq_files_begin(static_cast<const uint8_t*>(d_data), offs, lens, n, bits, max_size, s, &g.p);
  if (rc == SF_OK) rc = zpaq_files_finish(&g.p, max_rounds, s);
  if (rc != SF_OK) return rc;
  const uint64_t st[6] = {g.p.L, g.p.nseg, g.p.launches, g.p.recut, g.p.n_unsettled, 0};
  for (int k = 0; k < 6; k++) zpaq_files_stat(k, st[k]);
  *n_blocks = g.p.total;
  if (n_unsettled) *n_unsettled = g.p.n_unsettled;
  if (unsettled) memcpy(unsettled, g.p.unsettled.data(), n);
  if (g.p.total > cap_blocks || !d_offsets || !d_sizes || !d_first_row || !have_rest) return SF_ENOSPC;
  return zpaq_files_emit(g.p, d_offsets, d_sizes, d_first_row, s);
}

}  // namespace

extern "C" {

int sf_cut_device_zpaq_files(const void* d_data, uint64_t data_len, const uint64_t* file_offsets,
                             const uint64_t* file_lens, uint32_t n_files, uint32_t bits, uint32_t max_size,
                             uint32_t max_rounds, uint64_t* d_offsets, uint32_t* d_sizes, uint64_t cap_blocks,
                             uint64_t* d_first_row, uint64_t* n_blocks, uint8_t* unsettled, uint32_t* n_unsettled,
                             uint32_t* bad_file, void* stream) {
  return guarded([&] {
    return cut_files(d_data, data_len, file_offsets, file_lens, n_files, bits, max_size, max_rounds, d_offsets, d_sizes,
                     cap_blocks, d_first_row, true, n_blocks, unsettled, n_unsettled, bad_file, as_stream(stream));
  });
}

int sf_index_device_zpaq_files(const void* d_data, uint64_t data_len, const uint64_t* file_offsets,
                               const uint64_t* file_lens, uint32_t n_files, uint32_t bits, uint32_t max_size,
                               uint32_t max_rounds, uint64_t* d_offsets, uint32_t* d_sizes, void* d_digests,
                               uint64_t cap_blocks, uint64_t* d_first_row, uint64_t* n_blocks, uint8_t* blocks_hashes,
                               uint8_t* unsettled, uint32_t* n_unsettled, uint32_t* bad_file, void* stream) {
  return guarded([&]() -> int {
    hipStream_t s = as_stream(stream);
    if (misaligned(d_digests, 4)) {  // digests are written as dwords (Sha1::store)
      if (n_blocks) *n_blocks = 0;
      if (n_unsettled) *n_unsettled = 0;
      if (bad_file) *bad_file = 0;
      return SF_EINVAL;
    }
    std::vector<uint8_t> mask;
    if (blocks_hashes && !unsettled && n_files) {  // the chains below need the mask
      mask.resize(n_files);
      unsettled = mask.data();
    }
    int rc = cut_files(d_data, data_len, file_offsets, file_lens, n_files, bits, max_size, max_rounds, d_offsets,
                       d_sizes, cap_blocks, d_first_row, d_digests != nullptr, n_blocks, unsettled, n_unsettled,
                       bad_file, s);
    if (rc != SF_OK) return rc;
    const uint64_t n = *n_blocks;
    if (n && (rc = launch_table(d_data, data_len, d_offsets, d_sizes, n, d_digests, nullptr, s)) != SF_OK) return rc;
    if (!blocks_hashes || !n_files) return SF_OK;
    // every file's chain on the host, over its own rows' digests
    std::vector<uint8_t> dig(n * 20);
    std::vector<uint64_t> first((size_t)n_files + 1, 0);
    if (n) {
      SF_HIP(hipMemcpyAsync(dig.data(), d_digests, n * 20, hipMemcpyDeviceToHost, s));
      SF_HIP(hipMemcpyAsync(first.data(), d_first_row, first.size() * 8, hipMemcpyDeviceToHost, s));
      SF_HIP(hipStreamSynchronize(s));
    }
    for (uint32_t f = 0; f < n_files; f++) {
      uint8_t* out = blocks_hashes + (size_t)f * SF_HASH_DIGEST_LEN;
      if (unsettled[f]) {
        memset(out, 0, SF_HASH_DIGEST_LEN);
        continue;
      }
      if ((rc = sf_blocks_hash(dig.data() + first[f] * 20, first[f + 1] - first[f], out)) != SF_OK) return rc;
    }
    return SF_OK;
  });
}

int sf_test_zpaq_files_stats(uint64_t out[6]) {
  if (!out) return SF_EINVAL;
  for (int k = 0; k < 6; k++) out[k] = g_files_stats[k].load(std::memory_order_relaxed);
  return SF_OK;
}

}  // extern "C"
