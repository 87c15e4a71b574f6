// sf_serve_files.hip -- the source's side of the GET_FILE requests on the
// device (include/syncfast_amd.h: sf_wire_parse_get_files_device,
// sf_serve_get_files_device): a received request run parsed as the reference
// parser reads it, every name looked up in the source's name set, and the whole
// answer -- FILE_START, FILE_BLOCKs, FILE_END per request -- built in HBM from
// the index's own block table (src/sync/fs.rs:177-231).  The GET_FILE sibling
// of sf_send.hip's sf_serve_get_blocks_device.  Its own translation unit: the
// other kernels' code objects stay as they are.  The rules and the plan's
// arithmetic are sf_wire_get_files.hpp's, shared with the host test that
// executes them; the places of the messages are sf_wire_send_files.hpp's.
//
// The parse.  A request is two lines (sf_wire_get_files.hpp), so no message
// start is guessed:
//
//   newlines, scan   sf_recv_scan.hpp's candidates kernel and scan with the
//               rule "a '\n' stands here": the bitmap of the newlines, and
//               every newline's index -- its line's -- in position order.
//   lines       one lane per bitmap word: each of its newlines ends line j at p;
//               the line's length comes from the 128 bitmap bits below p (a
//               longer line fails either test), an even line must be the 8
//               bytes "GET_FILE", an odd one at most 100 bytes.  The first
//               failing line is an atomicMin, one atomic per wave.
//   extract     one lane per word: with K = min(first failing line, lines) / 2
//               requests, the newline of odd line j < 2K ends the name of
//               request j / 2: its span is written, bad_name lowered when it
//               is no UTF-8 (one atomic per wave); the last one writes the
//               consumed bytes and the bytes that stand there.
//   (read-back 1: K, consumed, bad_name and those bytes; the host classifies
//   the stop with classify_get_files)
//
// The answer, every dependency a kernel boundary:
//
//   lookup      sf_name_set_lookup over the spans just written.
//   counts      one lane per request: its row's CSR entries tested, its block
//               count and name length widened; the first unknown request and
//               the first bad row are an atomicMin each, one per wave.
//   scans       exclusive 64-bit scans: the request CSR over the answer's
//               blocks (req_first) and over its name bytes (name_off).
//   coarse      one lane per request: whether the answers up to and with it
//               leave 2^32 messages, or max_run_bytes with every block at its
//               shortest (34 bytes): bounds the blocks whose lengths are
//               scanned at all, whatever a hostile peer repeats.
//   decide      one lane: Kc = the first of those stops, Mc = req_first[Kc].
//   (read-back 2: Kc, Mc)
//   gather      one lane per block of the first Kc answers: its request by the
//               upper-bound search of req_first, its size from the table
//               through request -> row -> block, in answer order.
//   plan        sfi::wire_plan (sf_wire.hip): the FILE_BLOCK lengths and their
//               inclusive 64-bit scan E.
//   cut, final  one lane per request: the exact test against max_run_bytes;
//               one lane: n_answered and the run's three totals.
//   (read-back 3: n_answered, blocks, block bytes, name bytes, answered bytes;
//   the run is allocated then)
//   frames      one lane per answered request: FILE_START with the name's bytes
//               read in place from the request run, FILE_END, byte stores.
//   blocks      one lane per block: its request by the same search, its digest
//               through the same indirection, FILE_BLOCK at block_at, byte
//               stores.
//
// No lane waits for another; every loop is bounded by a word's 64 bits, a
// message's bytes or a binary search's 33 steps.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "sf_recv_scan.hpp"
#include "sf_wire_get_files.hpp"
#include "../../include/syncfast_amd_test.h"

using namespace sfrs;

namespace {

constexpr uint64_t kMaxRequestRun = 1ull << 35;  // bytes per call: fewer than 2^32 requests
constexpr uint64_t kMaxPerLaunch = 1ull << 30;   // lanes per launch (grid x stays far below 2^31)
constexpr unsigned long long kNone = ~0ull;

// What the host reads back of a parse, in one copy.
struct Parsed {
  unsigned long long first_bad;  // the first terminated line that fails its test
  unsigned long long lines, msgs, end, bad_name;
  uint32_t tail_n, pad;
  uint8_t tail[sfwp::kGetFilesTail];  // the bytes at `end`
};
static_assert(offsetof(Parsed, first_bad) == 0 && sizeof(Parsed::first_bad) == 8 && sizeof(Parsed) <= 256,
              "sfrs::Scan::result: 256 bytes that begin with first_bad");

// What the host reads back of the answer's plan (read-backs 2 and 3).
struct Served {
  unsigned long long unknown, coarse, bad, full;  // start at all ones; bad = (request << 32) | row
  unsigned long long kc, mc;                      // decide
  unsigned long long na, ma, block_bytes, name_bytes, answered_bytes;  // final
};

// "A '\n' stands here" as a rule of the candidates kernel: the bitmap of the
// newlines and their running count.
struct NewlineRules {
  static constexpr uint32_t kFirst = '\n', kSecond = 0;
  static __device__ __forceinline__ uint32_t message(const uint8_t*, uint64_t, uint32_t*, uint64_t*) { return 1; }
};

// The smallest v among the wave's lanes with `bad`, to *first (which starts
// at all ones): one atomic per wave that has one.  v grows with the lane.
__device__ __forceinline__ void first_bad(bool bad, unsigned long long v, unsigned long long* first) {
  const unsigned long long m = __ballot(bad);
  if (m && (threadIdx.x & 63u) == (uint32_t)__ffsll(m) - 1) atomicMin(first, v);
}

// The 64 bitmap bits below position q: bit 63 is position q - 1, bit 0
// position q - 64 (0 where that is below 0).
__device__ __forceinline__ unsigned long long bits_below(const unsigned long long* __restrict__ words, uint64_t nw,
                                                         uint64_t q) {
  if (q >= 64) return bits_from(words, nw, q - 64);
  return q ? words[0] << (64 - q) : 0ull;
}

// The length of line j, which ends at the newline at p: the distance to the
// newline before it (line 0 begins at byte 0), 128 for anything longer than
// 127 bytes -- no test passes a line of more than 100.
__device__ __forceinline__ uint32_t line_len(const unsigned long long* __restrict__ words, uint64_t nw, uint64_t j,
                                             uint64_t p) {
  if (j == 0) return p > 127 ? 128u : (uint32_t)p;
  const unsigned long long hi = bits_below(words, nw, p);
  if (hi) return (uint32_t)__clzll((long long)hi);
  const unsigned long long lo = p >= 64 ? bits_below(words, nw, p - 64) : 0ull;
  return lo ? 64u + (uint32_t)__clzll((long long)lo) : 128u;
}

__global__ void __launch_bounds__(256) get_files_lines_kernel(const uint8_t* __restrict__ data,
                                                              const unsigned long long* __restrict__ words,
                                                              const uint64_t* __restrict__ ends, uint64_t nw,
                                                              Parsed* __restrict__ res) {
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long bad = kNone;
  if (w < nw) {
    unsigned long long m = words[w];
    uint64_t j = ends[w] - (uint64_t)__popcll(m);
    for (; m; m &= m - 1, j++) {
      const uint64_t p = (w << 6) + (uint64_t)(__ffsll((long long)m) - 1);
      if (!sfwp::line_ok(data, j, p, line_len(words, nw, j, p))) {
        bad = j;
        break;
      }
    }
  }
  first_bad(bad != kNone, bad, &res->first_bad);
}

__device__ __forceinline__ void copy_tail(const uint8_t* __restrict__ data, uint64_t n, uint64_t e,
                                          Parsed* __restrict__ res) {
  const uint32_t tn = n - e < sfwp::kGetFilesTail ? (uint32_t)(n - e) : sfwp::kGetFilesTail;
  for (uint32_t k = 0; k < tn; k++) res->tail[k] = data[e + k];
  res->tail_n = tn;
}

__global__ void __launch_bounds__(256) get_files_extract_kernel(const uint8_t* __restrict__ data, uint64_t n,
                                                                const unsigned long long* __restrict__ words,
                                                                const uint64_t* __restrict__ ends, uint64_t nw,
                                                                uint64_t* __restrict__ name_at,
                                                                uint32_t* __restrict__ name_len, uint64_t cap,
                                                                Parsed* __restrict__ res) {
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long bad = kNone;
  if (w < nw) {
    const uint64_t lines = ends[nw - 1];
    const uint64_t k = sfwp::requests_of_lines(lines, res->first_bad);  // (written one launch earlier)
    if (w == 0) {
      res->lines = lines;
      res->msgs = k;
      if (k == 0) copy_tail(data, n, 0, res);  // no request: what stands at byte 0
    }
    unsigned long long m = words[w];
    uint64_t j = ends[w] - (uint64_t)__popcll(m);
    for (; m && j < 2 * k; m &= m - 1, j++) {
      if (!(j & 1)) continue;
      const uint64_t p = (w << 6) + (uint64_t)(__ffsll((long long)m) - 1);
      const uint32_t len = line_len(words, nw, j, p);  // at most 100: the line passed
      const uint64_t i = j >> 1, a = p - len;
      if (i < cap) {
        name_at[i] = a;
        name_len[i] = len;
      }
      if (bad == kNone && !sfwp::utf8_ok(data + a, len)) bad = i;
      if (i == k - 1) {
        res->end = p + 1;
        copy_tail(data, n, p + 1, res);
      }
    }
  }
  first_bad(bad != kNone, bad, &res->bad_name);
}

// Requests [0, n) and one lane more, which closes the two lists the scans
// read: cnt[k] = the blocks of request k's row (0 for an unknown name and for
// a row whose entries do not hold: nothing of such a row is read later),
// nl[k] = its name's length.
__global__ void __launch_bounds__(256) serve_counts_kernel(const int64_t* __restrict__ rows,
                                                           const uint32_t* __restrict__ name_len,
                                                           const uint64_t* __restrict__ first, uint64_t n_blocks,
                                                           uint64_t n, uint64_t* __restrict__ cnt,
                                                           uint64_t* __restrict__ nl, Served* __restrict__ sv) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool unknown = false, bad = false;
  uint64_t c = 0, l = 0;
  unsigned long long badv = kNone;
  if (k < n) {
    const int64_t r = rows[k];
    l = name_len[k];
    if (r < 0) {
      unknown = true;
    } else if (!sfwp::serve_row_ok(first, n_blocks, (uint64_t)r)) {
      bad = true;
      badv = (unsigned long long)k << 32 | (unsigned long long)r;
    } else {
      c = first[r + 1] - first[r];
    }
  }
  if (k <= n) {
    cnt[k] = c;
    nl[k] = l;
  }
  first_bad(unknown, k, &sv->unknown);
  first_bad(bad, badv, &sv->bad);
}

__global__ void __launch_bounds__(256) serve_coarse_kernel(const uint64_t* __restrict__ req_first,
                                                           const uint64_t* __restrict__ name_off, uint64_t n,
                                                           uint64_t max_run_bytes, Served* __restrict__ sv) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool over = false;
  if (k < n) {
    const uint64_t b = req_first[k + 1];
    over = sfwp::serve_over(b, sfwp::serve_coarse_bytes(b), name_off[k + 1], k + 1, max_run_bytes);
  }
  first_bad(over, k, &sv->coarse);
}

__device__ __forceinline__ unsigned long long min_ull(unsigned long long a, unsigned long long b) {
  return a < b ? a : b;
}

// One lane.
__global__ void serve_decide_kernel(const uint64_t* __restrict__ req_first, uint64_t n, uint64_t bad_name,
                                    Served* __restrict__ sv) {
  unsigned long long kc = min_ull(min_ull(n, bad_name), min_ull(sv->unknown, sv->coarse));
  if (sv->bad != kNone) kc = min_ull(kc, sv->bad >> 32);
  sv->kc = kc;
  sv->mc = req_first[kc];
}

struct Table {
  const uint64_t* first;    // the source's CSR: row r owns blocks [first[r], first[r + 1])
  const uint8_t* digests;   // n_blocks x 20
  const uint32_t* sizes;
};

// Blocks [base, base + n) of the first kc answers, in answer order.
__global__ void __launch_bounds__(256) serve_gather_kernel(Table t, const int64_t* __restrict__ rows,
                                                           const uint64_t* __restrict__ req_first, uint64_t kc,
                                                           uint64_t base, uint64_t n, uint32_t* __restrict__ sizes) {
  const uint64_t j = base + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= base + n) return;
  const uint64_t k = sfwp::file_of_block(req_first, kc, j);
  sizes[j] = t.sizes[sfwp::serve_block_src(t.first, req_first, rows, k, j)];
}

__global__ void __launch_bounds__(256) serve_cut_kernel(const uint64_t* __restrict__ req_first,
                                                        const uint64_t* __restrict__ name_off,
                                                        const uint64_t* __restrict__ ends, uint64_t n,
                                                        uint64_t max_run_bytes, Served* __restrict__ sv) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool over = false;
  if (k < n) {
    const uint64_t b = req_first[k + 1];
    over = sfwp::serve_over(b, sfwp::bex(ends, b), name_off[k + 1], k + 1, max_run_bytes);
  }
  first_bad(over, k, &sv->full);
}

// One lane.
__global__ void serve_final_kernel(const uint64_t* __restrict__ req_first, const uint64_t* __restrict__ name_off,
                                   const uint64_t* __restrict__ ends, const uint64_t* __restrict__ name_at,
                                   const uint32_t* __restrict__ name_len, Served* __restrict__ sv) {
  const unsigned long long na = min_ull(sv->kc, sv->full);
  const uint64_t ma = req_first[na];
  sv->na = na;
  sv->ma = ma;
  sv->block_bytes = sfwp::bex(ends, ma);
  sv->name_bytes = name_off[na];
  sv->answered_bytes = na ? name_at[na - 1] + name_len[na - 1] + 1 : 0;
}

__global__ void __launch_bounds__(256) serve_frames_kernel(const uint8_t* __restrict__ req,
                                                           const uint64_t* __restrict__ name_at,
                                                           const uint32_t* __restrict__ name_len,
                                                           const uint64_t* __restrict__ req_first,
                                                           const uint64_t* __restrict__ name_off,
                                                           const uint64_t* __restrict__ ends, uint64_t base, uint64_t n,
                                                           uint8_t* __restrict__ out) {
  const uint64_t k = base + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= base + n) return;
  sfwp::write_file_start(out + sfwp::start_at(ends, req_first, name_off, k), req + name_at[k], name_len[k]);
  sfwp::write_file_end(out + sfwp::end_at(ends, req_first, name_off, k));
}

__global__ void __launch_bounds__(256) serve_blocks_kernel(Table t, const int64_t* __restrict__ rows,
                                                           const uint64_t* __restrict__ req_first,
                                                           const uint64_t* __restrict__ name_off, uint64_t na,
                                                           const uint32_t* __restrict__ sizes,
                                                           const uint64_t* __restrict__ ends, uint64_t base, uint64_t n,
                                                           uint8_t* __restrict__ out) {
  const uint64_t j = base + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= base + n) return;
  const uint64_t k = sfwp::file_of_block(req_first, na, j);
  const uint64_t src = sfwp::serve_block_src(t.first, req_first, rows, k, j);
  sfwp::write_file_block(out + sfwp::block_at(ends, name_off, k, j), t.digests + sfwp::kDigest * src, sizes[j]);
}

sfi::Stats4 g_serve_stats;  // sf_test_serve_files_stats: route, requests, answered, read-backs

}  // namespace

using namespace sfi;

namespace {

constexpr uint64_t kRouteNothing = 0, kRouteParsed = 1, kRouteBuilt = 2;

// d_wire[0, n) (n > 0) parsed on s: the first min(requests, cap) spans written,
// *h = what came back, *stop = the class of what stands behind the requests.
// Blocking: one read-back.
int parse_device(const uint8_t* d_wire, uint64_t n, uint64_t* d_name_at, uint32_t* d_name_len, uint64_t cap, Parsed* h,
                 int* stop, hipStream_t s) {
  Scan sc(s);
  int rc = scan_candidates<NewlineRules>(d_wire, n, s, &sc);
  if (rc != SF_OK) return rc;
  Parsed* res = static_cast<Parsed*>(sc.result);
  SF_HIP(hipMemsetAsync(&res->bad_name, 0xFF, 8, s));
  const dim3 gw = grid256(sc.nw);
  rc = launch(get_files_lines_kernel, gw, dim3(256), s, d_wire, sc.words, sc.ends, sc.nw, res);
  if (rc != SF_OK) return rc;
  rc = launch(get_files_extract_kernel, gw, dim3(256), s, d_wire, n, sc.words, sc.ends, sc.nw, d_name_at, d_name_len,
              cap, res);
  if (rc != SF_OK) return rc;
  SF_HIP(hipMemcpyAsync(h, res, sizeof(Parsed), hipMemcpyDeviceToHost, s));
  SF_HIP(hipStreamSynchronize(s));
  if (h->msgs == 0) h->end = 0;
  uint32_t len = 0, name_len = 0;
  *stop = sfwp::classify_get_files(h->tail, h->tail_n, &len, &name_len);
  // (never, by the rules: a whole request behind the last one)
  return *stop == sfwp::kRequest ? SF_EIO : SF_OK;
}

int parse_get_files(const void* d_wire, uint64_t n_bytes, uint64_t* d_name_at, uint32_t* d_name_len, uint64_t cap,
                    uint64_t* n_out, uint64_t* bad_name, uint64_t* consumed, int* stop, hipStream_t s) {
  if (n_out) *n_out = 0;
  if (bad_name) *bad_name = UINT64_MAX;
  if (consumed) *consumed = 0;
  if (stop) *stop = SF_WIRE_END;
  if (!n_out || !bad_name || !consumed || !stop || (n_bytes && !d_wire) || n_bytes > kMaxRequestRun) return SF_EINVAL;
  if (misaligned(d_name_at, 8) || misaligned(d_name_len, 4)) return SF_EINVAL;  // 8-B and dword stores
  if (n_bytes == 0) return SF_OK;
  const bool query = !d_name_at || !d_name_len;
  if (query) cap = 0;  // a query writes nothing
  Parsed h{};
  const int rc = parse_device(static_cast<const uint8_t*>(d_wire), n_bytes, d_name_at, d_name_len, cap, &h, stop, s);
  if (rc != SF_OK) return rc;
  *n_out = h.msgs;
  *bad_name = h.bad_name;
  *consumed = h.end;
  if (query) return h.msgs ? SF_ENOSPC : SF_OK;
  return h.msgs > cap ? SF_ENOSPC : SF_OK;
}

struct ServeArgs {
  const sf_name_set* set;
  Table t;
  uint64_t n_blocks;
  const uint8_t* d_requests;
  uint64_t n_bytes, max_run_bytes;
  sf_wire_run** run;
  uint64_t *n_requests, *n_answered, *answered_bytes;
  int* why;
  uint64_t *bad_row, *consumed;
  int* stop;
};

int why_of(uint64_t na, uint64_t n, uint64_t bad_name, uint64_t unknown) {
  if (na == n) return SF_SERVE_ALL;
  if (na == bad_name) return SF_SERVE_BAD_NAME;
  if (na == unknown) return SF_SERVE_UNKNOWN;
  return SF_SERVE_FULL;
}

// n_bytes > 0.  Blocking.
int serve_device(const ServeArgs& a, hipStream_t s) {
  const uint64_t cap = a.n_bytes / sfwp::kMinGetFile + 1;  // a request is at least 10 bytes
  ScratchLayout L0;
  const size_t at_at = L0.add(cap * 8), rows_at = L0.add(cap * 8), len_at = L0.add(cap * 4), sv_at = L0.add(sizeof(Served));
  Scratch q(s);
  int rc = stream_alloc(&q.p, L0.total(), s);
  if (rc != SF_OK) return rc;
  uint64_t* name_at = L0.at<uint64_t>(q.p, at_at);
  int64_t* rows = L0.at<int64_t>(q.p, rows_at);
  uint32_t* name_len = L0.at<uint32_t>(q.p, len_at);
  Served* sv = L0.at<Served>(q.p, sv_at);

  Parsed h{};
  rc = parse_device(a.d_requests, a.n_bytes, name_at, name_len, cap, &h, a.stop, s);
  if (rc != SF_OK) return rc;
  uint64_t readbacks = 1;
  const uint64_t n = h.msgs;
  *a.n_requests = n;
  *a.consumed = h.end;
  g_serve_stats.set(0, kRouteParsed);
  g_serve_stats.set(1, n);
  g_serve_stats.set(3, readbacks);
  if (n == 0) {
    *a.run = wire_run_empty();
    return SF_OK;
  }

  rc = sf_name_set_lookup(a.set, a.d_requests, a.n_bytes, name_at, name_len, n, rows, s);
  if (rc != SF_OK) return rc;
  size_t tmp = 0;
  uint64_t* const nul = nullptr;
  if ((rc = scan_exclusive(nullptr, tmp, nul, nul, 0, n + 1, s)) != SF_OK) return rc;
  ScratchLayout L1;
  const size_t cnt_at = L1.add((n + 1) * 8), nl_at = L1.add((n + 1) * 8), rf_at = L1.add((n + 1) * 8),
               no_at = L1.add((n + 1) * 8);
  Scratch w(s);
  if ((rc = stream_alloc(&w.p, L1.total() + tmp + 8, s)) != SF_OK) return rc;
  uint64_t* cnt = L1.at<uint64_t>(w.p, cnt_at);
  uint64_t* nl = L1.at<uint64_t>(w.p, nl_at);
  uint64_t* req_first = L1.at<uint64_t>(w.p, rf_at);
  uint64_t* name_off = L1.at<uint64_t>(w.p, no_at);
  void* scan_tmp = L1.at<void>(w.p, L1.total());
  SF_HIP(hipMemsetAsync(sv, 0xFF, 4 * 8, s));
  rc = launch(serve_counts_kernel, grid256(n + 1), dim3(256), s, rows, name_len, a.t.first, a.n_blocks, n, cnt, nl, sv);
  if (rc == SF_OK) rc = scan_exclusive(scan_tmp, tmp, cnt, req_first, 0, n + 1, s);
  if (rc == SF_OK) rc = scan_exclusive(scan_tmp, tmp, nl, name_off, 0, n + 1, s);
  if (rc == SF_OK) rc = launch(serve_coarse_kernel, grid256(n), dim3(256), s, req_first, name_off, n, a.max_run_bytes, sv);
  if (rc == SF_OK) rc = launch(serve_decide_kernel, dim3(1), dim3(1), s, req_first, n, h.bad_name, sv);
  if (rc != SF_OK) return rc;
  Served v{};
  SF_HIP(hipMemcpyAsync(&v, sv, sizeof(Served), hipMemcpyDeviceToHost, s));
  SF_HIP(hipStreamSynchronize(s));
  g_serve_stats.set(3, ++readbacks);
  const uint64_t bad_at = v.bad == kNone ? UINT64_MAX : v.bad >> 32;
  const uint64_t kc = v.kc, mc = v.mc;

  Scratch plan(s), gs(s);  // wire_plan's allocation (E first), the sizes in answer order
  const uint64_t* ends = nullptr;
  uint32_t* sizes = nullptr;
  uint64_t na = 0;
  if (kc) {
    if (mc) {
      if ((rc = stream_alloc(&gs.p, mc * 4, s)) != SF_OK) return rc;
      sizes = static_cast<uint32_t*>(gs.p);
      rc = for_pieces(mc, kMaxPerLaunch, [&](uint64_t base, uint64_t c) {
        return launch(serve_gather_kernel, grid256(c), dim3(256), s, a.t, rows, req_first, kc, base, c, sizes);
      });
      if (rc != SF_OK) return rc;
      uint64_t* e = nullptr;
      if ((rc = wire_plan(sizes, mc, &e, s)) != SF_OK) return rc;
      plan.p = e;
      ends = e;
    }
    rc = launch(serve_cut_kernel, grid256(kc), dim3(256), s, req_first, name_off, ends, kc, a.max_run_bytes, sv);
    if (rc == SF_OK) rc = launch(serve_final_kernel, dim3(1), dim3(1), s, req_first, name_off, ends, name_at, name_len, sv);
    if (rc != SF_OK) return rc;
    SF_HIP(hipMemcpyAsync(&v, sv, sizeof(Served), hipMemcpyDeviceToHost, s));
    SF_HIP(hipStreamSynchronize(s));
    g_serve_stats.set(3, ++readbacks);
    na = v.na;
  }
  // The stop at na, in the reference's order: the name's encoding, the lookup, then the row's entries.
  if (na < n && na != h.bad_name && na != v.unknown && na == bad_at) {
    *a.bad_row = v.bad & 0xFFFFFFFFull;
    return SF_EINVAL;
  }
  *a.n_answered = na;
  *a.answered_bytes = na ? v.answered_bytes : 0;
  *a.why = why_of(na, n, h.bad_name, v.unknown);
  g_serve_stats.set(2, na);
  if (na == 0) {
    *a.run = wire_run_empty();
    return SF_OK;
  }
  g_serve_stats.set(0, kRouteBuilt);
  sf_wire_run* run = nullptr;
  rc = wire_run_begin(sfwp::files_run_total(v.block_bytes, v.name_bytes, na), v.ma + 2 * na, s, &run);
  if (rc == SF_OK)
    rc = for_pieces(na, kMaxPerLaunch, [&](uint64_t base, uint64_t c) {
      return launch(serve_frames_kernel, grid256(c), dim3(256), s, a.d_requests, name_at, name_len, req_first, name_off,
                    ends, base, c, run->bytes);
    });
  if (rc == SF_OK)
    rc = for_pieces(v.ma, kMaxPerLaunch, [&](uint64_t base, uint64_t c) {
      return launch(serve_blocks_kernel, grid256(c), dim3(256), s, a.t, rows, req_first, name_off, na, sizes, ends, base,
                    c, run->bytes);
    });
  return wire_run_finish(run, rc, s, a.run);
}

int serve_get_files(const ServeArgs& a, hipStream_t s) {
  g_serve_stats.reset();
  g_serve_stats.set(0, kRouteNothing);
  if (a.run) *a.run = nullptr;
  if (a.n_requests) *a.n_requests = 0;
  if (a.n_answered) *a.n_answered = 0;
  if (a.answered_bytes) *a.answered_bytes = 0;
  if (a.why) *a.why = SF_SERVE_ALL;
  if (a.bad_row) *a.bad_row = UINT64_MAX;
  if (a.consumed) *a.consumed = 0;
  if (a.stop) *a.stop = SF_WIRE_END;
  if (!a.run || !a.n_requests || !a.n_answered || !a.answered_bytes || !a.why || !a.bad_row || !a.consumed || !a.stop)
    return SF_EINVAL;
  if (a.n_bytes > kMaxRequestRun || a.n_blocks > sfwp::kServeMaxMessages) return SF_EINVAL;
  // 8-B loads of the CSR, dword loads of the sizes; the digest table as everywhere
  if (misaligned(a.t.first, 8) || misaligned(a.t.digests, 4) || misaligned(a.t.sizes, 4)) return SF_EINVAL;
  if (a.n_bytes && (!a.set || !a.d_requests || !a.t.first)) return SF_EINVAL;
  if (a.n_bytes && a.n_blocks && (!a.t.digests || !a.t.sizes)) return SF_EINVAL;
  if (a.n_bytes == 0) {
    *a.run = wire_run_empty();
    return SF_OK;
  }
  return serve_device(a, s);
}

}  // namespace

extern "C" {

int sf_wire_parse_get_files_device(const void* d_wire, uint64_t n_bytes, uint64_t* d_name_at, uint32_t* d_name_len,
                                   uint64_t cap, uint64_t* n_out, uint64_t* bad_name, uint64_t* consumed, int* stop,
                                   void* stream) {
  return guarded([&] {
    return parse_get_files(d_wire, n_bytes, d_name_at, d_name_len, cap, n_out, bad_name, consumed, stop,
                           as_stream(stream));
  });
}

int sf_serve_get_files_device(const sf_name_set* set, const uint64_t* d_file_first, const void* d_digests,
                              const uint32_t* d_sizes, uint64_t n_blocks, const void* d_requests, uint64_t n_bytes,
                              uint64_t max_run_bytes, sf_wire_run** run, uint64_t* n_requests, uint64_t* n_answered,
                              uint64_t* answered_bytes, int* why, uint64_t* bad_row, uint64_t* consumed, int* stop,
                              void* stream) {
  return guarded([&]() -> int {
    const ServeArgs a{set,        {d_file_first, static_cast<const uint8_t*>(d_digests), d_sizes},
                      n_blocks,   static_cast<const uint8_t*>(d_requests),
                      n_bytes,    max_run_bytes,
                      run,        n_requests,
                      n_answered, answered_bytes,
                      why,        bad_row,
                      consumed,   stop};
    return serve_get_files(a, as_stream(stream));
  });
}

int sf_test_serve_files_stats(uint64_t out[4]) { return g_serve_stats.read(out); }

}  // extern "C"
